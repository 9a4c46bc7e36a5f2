// Quaternion rotation weight (quaternion_conv_rotation / quaternion_transpose_conv_rotation / quaternion_linear_rotation,
// quaternion_ops.py:174-388 of the reference) and its gradient.  The reference builds ONE real weight K from the four
// component tensors u = (r, i, j, k), element by element, and runs one real convolution / transposed convolution / matmul
// with it; those run on the algebra-1 kernels, these two memory-bound kernels make K and fold dK back onto u.
//
// Per component element, n = |u|, f = 2n (sic: the reference's factor, not 2/n^2):
//   E = I + f*Q(u),  Q = [[-(j^2+k^2),  ij + rk,     ik - rj  ],
//                         [ ij - rk,    -(i^2+k^2),  jk + ri  ],
//                         [ ik + rj,     jk - ri,   -(i^2+j^2)]]
// K[m*A + a][c*B + b][t] = E[m][c](a, b, t) for component tensors (A, B, *taps); with quaternion_format block row 0 and
// block column 0 are zero and E sits at block (m+1, c+1).  Gradient: dL/du = (sum G*Q) * 2u/n + f * sum G * dQ/du with
// G[m][c] the element's 9 entries of dK -- one thread per element, no atomics, the same bits every run.
#include "common.h"

namespace seld {

struct RotW {
    const float* p[4];
};
struct RotDW {
    float* p[4];
};

// E row-major (e[m*3 + c]) in the reference's operation order (its float32 result to rounding; no contraction to FMA)
__device__ __forceinline__ void rot_form(float r, float i, float j, float k, float e[9]) {
#pragma clang fp contract(off)
    const float f = 2.0f * sqrtf(r * r + i * i + j * j + k * k);
    const float si = f * (i * i), sj = f * (j * j), sk = f * (k * k);
    const float ri = f * r * i, rj = f * r * j, rk = f * r * k;
    const float ij = f * i * j, ik = f * i * k, jk = f * j * k;
    e[0] = 1.0f - (sj + sk); e[1] = ij + rk;           e[2] = ik - rj;
    e[3] = ij - rk;          e[4] = 1.0f - (si + sk);  e[5] = jk + ri;
    e[6] = ik + rj;          e[7] = jk - ri;           e[8] = 1.0f - (si + sj);
}

// d[0..3] = dL/d(r, i, j, k) from g[m*3 + c] = dL/dE[m][c]
__device__ __forceinline__ void rot_grad(float r, float i, float j, float k, const float g[9], float d[4]) {
    const float n = sqrtf(r * r + i * i + j * j + k * k);
    const float f = 2.0f * n;
    const float q = g[0] * -(j * j + k * k) + g[1] * (i * j + r * k) + g[2] * (i * k - r * j)
                  + g[3] * (i * j - r * k) + g[4] * -(i * i + k * k) + g[5] * (j * k + r * i)
                  + g[6] * (i * k + r * j) + g[7] * (j * k - r * i) + g[8] * -(i * i + j * j);
    const float s = 2.0f * q / n;
    const float a01 = g[1] + g[3], s01 = g[1] - g[3];      // G01 +- G10
    const float a02 = g[2] + g[6], s20 = g[6] - g[2];      // G02 + G20, G20 - G02
    const float a12 = g[5] + g[7], s12 = g[5] - g[7];      // G12 +- G21
    d[0] = s * r + f * (k * s01 + j * s20 + i * s12);
    d[1] = s * i + f * (j * a01 + k * a02 + r * s12 - 2.0f * i * (g[4] + g[8]));
    d[2] = s * j + f * (i * a01 + k * a12 + r * s20 - 2.0f * j * (g[0] + g[8]));
    d[3] = s * k + f * (r * s01 + i * a02 + j * a12 - 2.0f * k * (g[0] + g[4]));
}

// value of block (mb, cb) of an MB x MB block matrix (MB = 4: quaternion_format, zero row / column 0)
template <int MB>
__device__ __forceinline__ float rot_block(const float e[9], int mb, int cb) {
    constexpr int o = MB - 3;
    return (MB == 4 && (mb == 0 || cb == 0)) ? 0.0f : e[(mb - o) * 3 + cb - o];
}

// ---- SELD_ROT_LAYOUT_CONV: K (MB*A, MB*B, taps).  Thread e = a*BT + jj; every store of a block is a contiguous run
// along the (b, t) index jj, as are the component loads.
template <int MB>
__global__ __launch_bounds__(256) void rot_form_kernel(RotW w, float* __restrict__ K, long long A, long long BT) {
    const long long total = A * BT, row = MB * BT;
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long a = e / BT, jj = e - a * BT;
        float v[9];
        rot_form(w.p[0][e], w.p[1][e], w.p[2][e], w.p[3][e], v);
        float* base = K + a * row + jj;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int cb = 0; cb < MB; ++cb) base[mb * A * row + cb * BT] = rot_block<MB>(v, mb, cb);
    }
}

template <int MB>
__global__ __launch_bounds__(256) void rot_form_bwd_kernel(RotW w, const float* __restrict__ dK, RotDW dw, long long A,
                                                           long long BT, int accumulate) {
    constexpr int o = MB - 3;
    const long long total = A * BT, row = MB * BT;
    for (long long e = blockIdx.x * 256LL + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long a = e / BT, jj = e - a * BT;
        const float* base = dK + a * row + jj;
        float g[9], d[4];
#pragma unroll
        for (int m = 0; m < 3; ++m)
#pragma unroll
            for (int c = 0; c < 3; ++c) g[m * 3 + c] = base[(m + o) * A * row + (c + o) * BT];
        rot_grad(w.p[0][e], w.p[1][e], w.p[2][e], w.p[3][e], g, d);
#pragma unroll
        for (int c = 0; c < 4; ++c) dw.p[c][e] = accumulate ? dw.p[c][e] + d[c] : d[c];
    }
}

// ---- SELD_ROT_LAYOUT_LINEAR: W = K^T (MB*B, MB*A), components (A, B).  The components are contiguous along b, W along
// a: a 32 x 32 tile of the four components is staged through LDS (padded rows, no bank conflicts), loaded along b and
// used along a.
constexpr int ROT_TILE = 32;

template <int MB>
__global__ __launch_bounds__(256) void rot_form_t_kernel(RotW w, float* __restrict__ K, int A, int B) {
    __shared__ float s[4][ROT_TILE][ROT_TILE + 1];
    const int a0 = blockIdx.y * ROT_TILE, b0 = blockIdx.x * ROT_TILE;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int q = 0; q < ROT_TILE; q += 8) {
        const int a = a0 + ty + q, b = b0 + tx;
        if (a < A && b < B) {
            const long long e = (long long)a * B + b;
#pragma unroll
            for (int c = 0; c < 4; ++c) s[c][ty + q][tx] = w.p[c][e];
        }
    }
    __syncthreads();
    const long long row = (long long)MB * A;
#pragma unroll
    for (int q = 0; q < ROT_TILE; q += 8) {
        const int a = a0 + tx, b = b0 + ty + q;
        if (a < A && b < B) {
            float v[9];
            rot_form(s[0][tx][ty + q], s[1][tx][ty + q], s[2][tx][ty + q], s[3][tx][ty + q], v);
            float* base = K + (long long)b * row + a;
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int cb = 0; cb < MB; ++cb) base[(long long)cb * B * row + mb * A] = rot_block<MB>(v, mb, cb);
        }
    }
}

template <int MB>
__global__ __launch_bounds__(256) void rot_form_t_bwd_kernel(RotW w, const float* __restrict__ dK, RotDW dw, int A, int B,
                                                             int accumulate) {
    constexpr int o = MB - 3;
    __shared__ float s[4][ROT_TILE][ROT_TILE + 1];
    const int a0 = blockIdx.y * ROT_TILE, b0 = blockIdx.x * ROT_TILE;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int q = 0; q < ROT_TILE; q += 8) {
        const int a = a0 + ty + q, b = b0 + tx;
        if (a < A && b < B) {
            const long long e = (long long)a * B + b;
#pragma unroll
            for (int c = 0; c < 4; ++c) s[c][ty + q][tx] = w.p[c][e];
        }
    }
    __syncthreads();
    const long long row = (long long)MB * A;
#pragma unroll
    for (int q = 0; q < ROT_TILE; q += 8) {
        const int a = a0 + tx, b = b0 + ty + q;
        if (a < A && b < B) {
            const float* base = dK + (long long)b * row + a;
            float g[9], d[4];
#pragma unroll
            for (int m = 0; m < 3; ++m)
#pragma unroll
                for (int c = 0; c < 3; ++c) g[m * 3 + c] = base[(long long)(c + o) * B * row + (m + o) * A];
            rot_grad(s[0][tx][ty + q], s[1][tx][ty + q], s[2][tx][ty + q], s[3][tx][ty + q], g, d);
#pragma unroll
            for (int c = 0; c < 4; ++c) s[c][tx][ty + q] = d[c];       // this thread's own element: no hazard
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < ROT_TILE; q += 8) {
        const int a = a0 + ty + q, b = b0 + tx;
        if (a < A && b < B) {
            const long long e = (long long)a * B + b;
#pragma unroll
            for (int c = 0; c < 4; ++c) dw.p[c][e] = accumulate ? dw.p[c][e] + s[c][ty + q][tx] : s[c][ty + q][tx];
        }
    }
}

static int rot_check(int32_t layout, int32_t qformat, int32_t A, int32_t B, int32_t taps) {
    if (layout != SELD_ROT_LAYOUT_CONV && layout != SELD_ROT_LAYOUT_LINEAR) return SELD_EINVAL;
    if ((qformat != 0 && qformat != 1) || A <= 0 || B <= 0 || taps <= 0) return SELD_EINVAL;
    if (layout == SELD_ROT_LAYOUT_LINEAR && (taps != 1 || (A + ROT_TILE - 1) / ROT_TILE > 65535)) return SELD_EINVAL;
    return SELD_OK;
}

static dim3 rot_grid(long long total) {
    long long g = (total + 255) / 256;
    return dim3((unsigned)(g < 1 ? 1 : (g > 4096 ? 4096 : g)));
}

}  // namespace seld

using namespace seld;

extern "C" int seld_quat_rotation_form(int32_t layout, int32_t qformat, int32_t A, int32_t B, int32_t taps,
                                       const float* const w[4], float* K, void* stream) {
    int rc = rot_check(layout, qformat, A, B, taps);
    if (rc) return rc;
    if (!w || !w[0] || !w[1] || !w[2] || !w[3] || !K) return SELD_EINVAL;
    const RotW rw{{w[0], w[1], w[2], w[3]}};
    hipStream_t st = (hipStream_t)stream;
    if (layout == SELD_ROT_LAYOUT_CONV) {
        const long long BT = (long long)B * taps;
        const dim3 grid = rot_grid((long long)A * BT);
        if (qformat) hipLaunchKernelGGL(rot_form_kernel<4>, grid, dim3(256), 0, st, rw, K, (long long)A, BT);
        else hipLaunchKernelGGL(rot_form_kernel<3>, grid, dim3(256), 0, st, rw, K, (long long)A, BT);
    } else {
        const dim3 grid((B + ROT_TILE - 1) / ROT_TILE, (A + ROT_TILE - 1) / ROT_TILE);
        if (qformat) hipLaunchKernelGGL(rot_form_t_kernel<4>, grid, dim3(256), 0, st, rw, K, A, B);
        else hipLaunchKernelGGL(rot_form_t_kernel<3>, grid, dim3(256), 0, st, rw, K, A, B);
    }
    return check_launch();
}

extern "C" int seld_quat_rotation_form_bwd(int32_t layout, int32_t qformat, int32_t A, int32_t B, int32_t taps,
                                           const float* const w[4], const float* dK, float* const dw[4],
                                           int32_t accumulate, void* stream) {
    int rc = rot_check(layout, qformat, A, B, taps);
    if (rc) return rc;
    if (!w || !w[0] || !w[1] || !w[2] || !w[3] || !dK || !dw || !dw[0] || !dw[1] || !dw[2] || !dw[3]) return SELD_EINVAL;
    if (accumulate != 0 && accumulate != 1) return SELD_EINVAL;
    const RotW rw{{w[0], w[1], w[2], w[3]}};
    const RotDW rd{{dw[0], dw[1], dw[2], dw[3]}};
    hipStream_t st = (hipStream_t)stream;
    if (layout == SELD_ROT_LAYOUT_CONV) {
        const long long BT = (long long)B * taps;
        const dim3 grid = rot_grid((long long)A * BT);
        if (qformat) hipLaunchKernelGGL(rot_form_bwd_kernel<4>, grid, dim3(256), 0, st, rw, dK, rd, (long long)A, BT, accumulate);
        else hipLaunchKernelGGL(rot_form_bwd_kernel<3>, grid, dim3(256), 0, st, rw, dK, rd, (long long)A, BT, accumulate);
    } else {
        const dim3 grid((B + ROT_TILE - 1) / ROT_TILE, (A + ROT_TILE - 1) / ROT_TILE);
        if (qformat) hipLaunchKernelGGL(rot_form_t_bwd_kernel<4>, grid, dim3(256), 0, st, rw, dK, rd, A, B, accumulate);
        else hipLaunchKernelGGL(rot_form_t_bwd_kernel<3>, grid, dim3(256), 0, st, rw, dK, rd, A, B, accumulate);
    }
    return check_launch();
}
