// Plain activations, add / accumulate, max pooling, Philox dropout (with the first stage's BatchNorm + ReLU finish and the
// row masks) and the (N, C, T) <-> (N, T, C) transposes for gfx950.  All HBM-bound grid-stride kernels.
#include "nn_common.h"

namespace seld {

// ------------------------------------------------------------------------------------------
// plain activations, add
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void act_fwd_kernel(const float* __restrict__ x, long long n, int act,
                                                      float* __restrict__ y) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        y[i] = act_apply(x[i], act);
}
__global__ __launch_bounds__(256) void act_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                                      long long n, int act, float* __restrict__ dx) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        dx[i] = dy[i] * act_grad_from_y(y[i], act);
}
__global__ __launch_bounds__(256) void add_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                  long long n, float* __restrict__ y) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        y[i] = a[i] + b[i];
}

// ------------------------------------------------------------------------------------------
// max pooling, window == stride, floor mode.  x (NC, H, W) -> y (NC, H/ph, W/pw)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* __restrict__ x, long long NC, int H, int W,
                                                          int ph, int pw, int OH, int OW, float* __restrict__ y,
                                                          uint8_t* __restrict__ idx) {
    const long long total = NC * OH * OW;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int ow = (int)(i % OW);
        const long long t = i / OW;
        const int oh = (int)(t % OH);
        const long long nc = t / OH;
        const float* base = x + ((size_t)nc * H + (size_t)oh * ph) * W + (size_t)ow * pw;
        float best = base[0];
        int bi = 0;
        for (int a = 0; a < ph; ++a)
            for (int b = 0; b < pw; ++b) {
                const float v = base[(size_t)a * W + b];
                if (v > best || v != v) {   // first maximum wins; NaN propagates (torch semantics)
                    best = v;
                    bi = a * pw + b;
                }
            }
        y[i] = best;
        if (idx) idx[i] = (uint8_t)bi;
    }
}

__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ dy, const uint8_t* __restrict__ idx,
                                                          long long NC, int H, int W, int ph, int pw, int OH, int OW,
                                                          float* __restrict__ dx) {
    const long long total = NC * H * W;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int w = (int)(i % W);
        const long long t = i / W;
        const int h = (int)(t % H);
        const long long nc = t / H;
        const int oh = h / ph, ow = w / pw;
        float v = 0.f;
        if (oh < OH && ow < OW) {
            const size_t o = ((size_t)nc * OH + oh) * OW + ow;
            const int local = (h - oh * ph) * pw + (w - ow * pw);
            if (idx[o] == local) v = dy[o];
        }
        dx[i] = v;
    }
}

// ------------------------------------------------------------------------------------------
// Philox-4x32-10 dropout
// ------------------------------------------------------------------------------------------
// philox4x32_10 / u01: common.h

// `state` (nullable): the device-resident step state of seld_step_begin; state[0] is added to `offset`, so that a
// launch recorded in a HIP graph draws fresh numbers at every replay.
__global__ __launch_bounds__(256) void dropout_kernel(const float* __restrict__ x, long long n, float p, float scale,
                                                      uint64_t seed, uint64_t offset, const uint64_t* __restrict__ state,
                                                      float* __restrict__ y) {
    if (state) offset += state[0];
    const long long groups = (n + 3) >> 2;
    for (long long gi = (long long)blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += (long long)gridDim.x * blockDim.x) {
        const uint4 r = philox4x32_10(offset + (uint64_t)gi, seed);
        const uint32_t rr[4] = {r.x, r.y, r.z, r.w};
        const long long i = gi << 2;
        if (i + 3 < n) {
            float4 v = *reinterpret_cast<const float4*>(x + i);
            v.x = u01(rr[0]) >= p ? v.x * scale : 0.f;
            v.y = u01(rr[1]) >= p ? v.y * scale : 0.f;
            v.z = u01(rr[2]) >= p ? v.z * scale : 0.f;
            v.w = u01(rr[3]) >= p ? v.w * scale : 0.f;
            *reinterpret_cast<float4*>(y + i) = v;
        } else {
            for (int k = 0; k < 4 && i + k < n; ++k) y[i + k] = u01(rr[k]) >= p ? x[i + k] * scale : 0.f;
        }
    }
}

// pooled = relu(a * raw + b) on the pooled-size tensor the pooling convolution kernel left (hcq_first_pool_kernel), and --
// the stage's Dropout (model.py:282) in the same pass -- out = dropout(pooled) with exactly the mask dropout_kernel would
// draw for the same (seed, offset): group gi = linear element index / 4.  One workgroup per (n, c) plane.
__global__ __launch_bounds__(256) void bn_pool_finish_kernel(const float* __restrict__ raw, int C, int S,
                                                             const float* __restrict__ mean, const float* __restrict__ invstd,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             float* __restrict__ pooled, float p, float scale, uint64_t seed,
                                                             uint64_t offset, const uint64_t* __restrict__ state,
                                                             float* __restrict__ out) {
    const int c = blockIdx.x % C;
    const float a = gamma[c] * invstd[c], b = beta[c] - mean[c] * a;
    const size_t base = (size_t)blockIdx.x * S;
    if (out && state) offset += state[0];
    for (int s = threadIdx.x * 4; s < S; s += 256 * 4) {
        const float4 v = *reinterpret_cast<const float4*>(raw + base + s);
        float4 o;
        o.x = fmaxf(v.x * a + b, 0.f); o.y = fmaxf(v.y * a + b, 0.f);
        o.z = fmaxf(v.z * a + b, 0.f); o.w = fmaxf(v.w * a + b, 0.f);
        if (v.x != v.x) o.x = v.x;                                   // NaN propagates (torch's relu / max_pool)
        if (v.y != v.y) o.y = v.y;
        if (v.z != v.z) o.z = v.z;
        if (v.w != v.w) o.w = v.w;
        if (pooled) *reinterpret_cast<float4*>(pooled + base + s) = o;
        if (out) {
            const uint4 r = philox4x32_10(offset + (uint64_t)((base + s) >> 2), seed);
            float4 d;
            d.x = u01(r.x) >= p ? o.x * scale : 0.f;
            d.y = u01(r.y) >= p ? o.y * scale : 0.f;
            d.z = u01(r.z) >= p ? o.z * scale : 0.f;
            d.w = u01(r.w) >= p ? o.w * scale : 0.f;
            *reinterpret_cast<float4*>(out + base + s) = d;
        }
    }
}

__global__ void dropout_mask_rows_kernel(long long rows, float p, float scale, uint64_t seed, uint64_t offset,
                                         const uint64_t* __restrict__ state, float* __restrict__ mask) {
    if (state) offset += state[0];
    const long long groups = (rows + 3) >> 2;
    for (long long gi = (long long)blockIdx.x * blockDim.x + threadIdx.x; gi < groups; gi += (long long)gridDim.x * blockDim.x) {
        const uint4 r = philox4x32_10(offset + (uint64_t)gi, seed);
        const uint32_t rr[4] = {r.x, r.y, r.z, r.w};
        for (int k = 0; k < 4 && gi * 4 + k < rows; ++k) mask[gi * 4 + k] = u01(rr[k]) >= p ? scale : 0.f;
    }
}

// ------------------------------------------------------------------------------------------
// (N, C, T) <-> (N, T, C)
// ------------------------------------------------------------------------------------------
__global__ void transpose_kernel(const float* __restrict__ x, int R, int Cc, float* __restrict__ y) {
    // per batch item: x (R, Cc) -> y (Cc, R)
    __shared__ float tile[32][33];
    const size_t base = (size_t)blockIdx.z * R * Cc;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        const int r = r0 + j, c = c0 + threadIdx.x;
        if (r < R && c < Cc) tile[j][threadIdx.x] = x[base + (size_t)r * Cc + c];
    }
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += blockDim.y) {
        const int c = c0 + j, r = r0 + threadIdx.x;
        if (r < R && c < Cc) y[base + (size_t)c * R + r] = tile[threadIdx.x][j];
    }
}

}  // namespace seld

using namespace seld;

extern "C" int seld_act_fwd(const float* x, int64_t n, int32_t act, float* y, void* stream) {
    if (!x || !y || n < 0) return SELD_EINVAL;
    if (n == 0) return SELD_OK;
    hipLaunchKernelGGL(act_fwd_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), x, (long long)n, act, y);
    return check_launch();
}
extern "C" int seld_act_bwd(const float* dy, const float* y, int64_t n, int32_t act, float* dx, void* stream) {
    if (!dy || !y || !dx || n < 0) return SELD_EINVAL;
    if (n == 0) return SELD_OK;
    hipLaunchKernelGGL(act_bwd_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), dy, y, (long long)n, act, dx);
    return check_launch();
}
extern "C" int seld_accumulate(float* dst, const float* src, int64_t n, void* stream) {
    if (!dst || !src || n < 0) return SELD_EINVAL;
    if (n == 0) return SELD_OK;
    hipLaunchKernelGGL(add_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), (const float*)dst, src, (long long)n, dst);
    return check_launch();
}

extern "C" int seld_add(const float* a, const float* b, int64_t n, float* y, void* stream) {
    if (!a || !b || !y || n < 0) return SELD_EINVAL;
    if (n == 0) return SELD_OK;
    hipLaunchKernelGGL(add_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), a, b, (long long)n, y);
    return check_launch();
}

extern "C" int seld_maxpool_fwd(const float* x, int64_t NC, int32_t H, int32_t W, int32_t ph, int32_t pw, float* y,
                                uint8_t* idx, void* stream) {
    if (!x || !y || ph <= 0 || pw <= 0 || ph * pw > 255 || H < ph || W < pw) return SELD_EINVAL;
    const int OH = H / ph, OW = W / pw;
    hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(grid_for(NC * OH * OW)), dim3(256), 0, ST(stream), x, (long long)NC, H, W,
                       ph, pw, OH, OW, y, idx);
    return check_launch();
}
extern "C" int seld_maxpool_bwd(const float* dy, const uint8_t* idx, int64_t NC, int32_t H, int32_t W, int32_t ph,
                                int32_t pw, float* dx, void* stream) {
    if (!dy || !idx || !dx || ph <= 0 || pw <= 0 || H < ph || W < pw) return SELD_EINVAL;
    const int OH = H / ph, OW = W / pw;
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(grid_for(NC * H * W)), dim3(256), 0, ST(stream), dy, idx, (long long)NC, H,
                       W, ph, pw, OH, OW, dx);
    return check_launch();
}

extern "C" int seld_dropout_fwd(const float* x, int64_t n, float p, uint64_t seed, uint64_t offset,
                                const uint64_t* state, float* y, void* stream) {
    if (!x || !y || n < 0 || p < 0.f || p >= 1.f) return SELD_EINVAL;
    if (n == 0) return SELD_OK;
    hipLaunchKernelGGL(dropout_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, ST(stream), x, (long long)n, p,
                       1.0f / (1.0f - p), seed, offset, state, y);
    return check_launch();
}
extern "C" int seld_bn_pool_finish(const float* raw, int32_t N, int32_t C, int32_t S, const float* mean, const float* invstd,
                                   const float* gamma, const float* beta, float* pooled, float p, uint64_t seed,
                                   uint64_t offset, const uint64_t* state, float* out, void* stream) {
    if (!raw || !mean || !invstd || !gamma || !beta || (!pooled && !out) || N <= 0 || C <= 0 || S <= 0 || (S & 3)) return SELD_EINVAL;
    if (out && (p < 0.f || p >= 1.f)) return SELD_EINVAL;
    hipLaunchKernelGGL(bn_pool_finish_kernel, dim3((unsigned)(N * C)), dim3(256), 0, ST(stream), raw, C, S, mean, invstd,
                       gamma, beta, pooled, p, out ? 1.0f / (1.0f - p) : 1.0f, seed, offset, state, out);
    return check_launch();
}

extern "C" int seld_dropout_mask_rows(int64_t rows, float p, uint64_t seed, uint64_t offset, const uint64_t* state,
                                      float* mask, void* stream) {
    if (!mask || rows <= 0 || p < 0.f || p >= 1.f) return SELD_EINVAL;
    hipLaunchKernelGGL(dropout_mask_rows_kernel, dim3(grid_for((rows + 3) / 4)), dim3(256), 0, ST(stream), (long long)rows,
                       p, 1.0f / (1.0f - p), seed, offset, state, mask);
    return check_launch();
}

extern "C" int seld_transpose_nct_ntc(const float* x, int32_t N, int32_t C, int32_t T, float* y, void* stream) {
    if (!x || !y || N <= 0 || C <= 0 || T <= 0) return SELD_EINVAL;
    dim3 grid((T + 31) / 32, (C + 31) / 32, N);
    hipLaunchKernelGGL(transpose_kernel, grid, dim3(32, 8), 0, ST(stream), x, C, T, y);
    return check_launch();
}
extern "C" int seld_transpose_ntc_nct(const float* x, int32_t N, int32_t T, int32_t C, float* y, void* stream) {
    if (!x || !y || N <= 0 || C <= 0 || T <= 0) return SELD_EINVAL;
    dim3 grid((C + 31) / 32, (T + 31) / 32, N);
    hipLaunchKernelGGL(transpose_kernel, grid, dim3(32, 8), 0, ST(stream), x, T, C, y);
    return check_launch();
}
