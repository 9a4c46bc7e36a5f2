// Squeeze-and-excitation for gfx950 (include/seld_hip.h has the definition): two HBM-bound passes over an (N, C, S)
// activation in each direction and a tiny per-sample MLP between them.
//
// The streaming kernels see the tensor as N*C rows of S floats and never divide per element: a row's gate is one scalar.
// The two that sum (squeeze, bwd_reduce) give every row one owner:
//   row form    S <  SELD_SE_BLOCK_MIN_S: one WAVE per row, four rows per 256-thread workgroup
//   block form  S >= SELD_SE_BLOCK_MIN_S: one 256-thread workgroup per row
// The two that write (scale, bwd_apply) take the chunk form: one wave per 256 floats of a row, one access per lane.
// A row starts at element row * S, which is 16-byte aligned only when S % 4 == 0: every row is walked as up to three head
// elements in front of its first 16-byte boundary, aligned groups of four, and up to three tail elements (row_walk).
// When the tensors of a call do not sit at the same offset from a 16-byte boundary the x1 forms walk single elements.
//
// No atomics anywhere.  A row's sum belongs to one wave or one workgroup and runs in a fixed order: per lane head element,
// then its groups in order (each group (a+b)+(c+d)), then its tail element; the 64 lanes by an xor butterfly (6 levels);
// in the block form the four waves' sums as ((w0+w1)+w2)+w3.  The sums over the batch index in the parameter gradients
// run n = 0, 1, ... in one thread.  Two runs give the same bytes.
#include <cstdio>

#include "common.h"

namespace seld {

// f1(i): element i of the row; f4(i): the aligned group i .. i+3.  `lane` of L lanes, all of the same row.
template <bool VEC, int L, typename F4, typename F1>
__device__ __forceinline__ void row_walk(const float* rowptr, int S, int lane, F4&& f4, F1&& f1) {
    if (VEC) {
        int head = (int)(((16u - (unsigned)((uintptr_t)rowptr & 15u)) & 15u) >> 2);
        if (head > S) head = S;
        const int groups = (S - head) >> 2;
        const int tail0 = head + 4 * groups;
        if (lane < head) f1(lane);
#pragma unroll 4
        for (int g = lane; g < groups; g += L) f4(head + 4 * g);
        if (lane < S - tail0) f1(tail0 + lane);
    } else {
        for (int i = lane; i < S; i += L) f1(i);
    }
}

// the sum of `v` over the workgroup's 256 threads, in every thread; `red` is 4 floats of LDS.  Ends on a barrier, so
// `red` can be reused by the next row.
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return r;
}

// rows handled by this wave (row form) or workgroup (block form): first, stride; and the lane index inside the row
template <bool BLOCK>
__device__ __forceinline__ void row_schedule(long long* first, long long* stride, int* lane) {
    if (BLOCK) {
        *first = blockIdx.x;
        *stride = gridDim.x;
        *lane = threadIdx.x;
    } else {
        *first = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
        *stride = (long long)gridDim.x * 4;
        *lane = threadIdx.x & 63;
    }
}

// rowsum[row] = sum_s x[row, s]
template <bool VEC, bool BLOCK>
__global__ __launch_bounds__(256) void se_squeeze_kernel(const float* __restrict__ x, long long rows, int S,
                                                         float* __restrict__ rowsum) {
    __shared__ float red[4];
    long long first, stride;
    int lane;
    row_schedule<BLOCK>(&first, &stride, &lane);
    for (long long row = first; row < rows; row += stride) {
        const float* xr = x + (size_t)row * S;
        float acc = 0.f;
        row_walk<VEC, BLOCK ? 256 : 64>(
            xr, S, lane,
            [&](int i) {
                const float4 a = *reinterpret_cast<const float4*>(xr + i);
                acc += (a.x + a.y) + (a.z + a.w);
            },
            [&](int i) { acc += xr[i]; });
        acc = BLOCK ? block_sum(acc, red) : wave_sum(acc);
        if (lane == 0) rowsum[row] = acc;
    }
}

// q[row] = sum_s dy[row, s] * x[row, s]
template <bool VEC, bool BLOCK>
__global__ __launch_bounds__(256) void se_bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                            long long rows, int S, float* __restrict__ q) {
    __shared__ float red[4];
    long long first, stride;
    int lane;
    row_schedule<BLOCK>(&first, &stride, &lane);
    for (long long row = first; row < rows; row += stride) {
        const float* xr = x + (size_t)row * S;
        const float* dr = dy + (size_t)row * S;
        float acc = 0.f;
        row_walk<VEC, BLOCK ? 256 : 64>(
            xr, S, lane,
            [&](int i) {
                const float4 a = *reinterpret_cast<const float4*>(xr + i);
                const float4 d = *reinterpret_cast<const float4*>(dr + i);
                acc += (d.x * a.x + d.y * a.y) + (d.z * a.z + d.w * a.w);
            },
            [&](int i) { acc += dr[i] * xr[i]; });
        acc = BLOCK ? block_sum(acc, red) : wave_sum(acc);
        if (lane == 0) q[row] = acc;
    }
}

// out[row, :] = a[row, :] * s[n, c mod Cg] + (add ? add[n, c mod Cg] * inv_as : 0): y = x * s, and dx = dy * s + dz / (A S).
// Nothing is summed, so a row needs no owner: one WAVE per chunk of a row -- 64 aligned groups of four (x4: chunk 0 also
// takes the row's head elements, the last chunk its tail) or 256 single elements (x1) -- and one access per lane, as the
// element walks of norm.hip have it, but with two scalar divisions per chunk instead of a 64-bit one per lane.
// The chunk index is 32 bits (a 64-bit division is emulated in about a hundred instructions and sits in front of the wave's
// first load; 2^32 chunks are 4 TiB of floats); element offsets are 64 bits.  log2A: A = 1, 4, 8 as a shift.
template <bool VEC>
__global__ __launch_bounds__(256) void se_scale_kernel(const float* __restrict__ a, unsigned items, int log2A, int Cg, int S,
                                                       int chunks, const float* __restrict__ s,
                                                       const float* __restrict__ add, float inv_as, float* __restrict__ out) {
    typedef unsigned I;
    const int lane = threadIdx.x & 63;
    for (I item = (I)blockIdx.x * 4 + (I)__builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6); item < items;
         item += (I)gridDim.x * 4) {
        // the divisions run on the vector unit: readfirstlane brings the (wave-uniform) results back to scalar registers,
        // so the two gate constants are scalar loads that do not queue behind the streaming traffic
        const I row = __builtin_amdgcn_readfirstlane(item / (I)chunks);
        const int chunk = (int)(item - row * (I)chunks);
        const I k = row / (I)Cg;                                    // row = (n A + component) Cg + g
        const I gate = __builtin_amdgcn_readfirstlane((k >> log2A) * (I)Cg + (row - k * (I)Cg));
        const float sv = s[gate];
        const float b = add ? add[gate] * inv_as : 0.f;
        const float* ar = a + (size_t)row * S;
        float* orow = out + (size_t)row * S;
        if (VEC) {
            int head = (int)(((16u - (unsigned)((uintptr_t)ar & 15u)) & 15u) >> 2);
            if (head > S) head = S;
            const int groups = (S - head) >> 2;
            const size_t tail0 = (size_t)head + 4 * (size_t)groups;
            if (chunk == 0 && lane < head) orow[lane] = ar[lane] * sv + b;
            const long long g = (long long)chunk * 64 + lane;
            if (g < groups) {
                const size_t i = (size_t)head + 4 * (size_t)g;
                float4 v = *reinterpret_cast<const float4*>(ar + i);
                v.x = v.x * sv + b;
                v.y = v.y * sv + b;
                v.z = v.z * sv + b;
                v.w = v.w * sv + b;
                *reinterpret_cast<float4*>(orow + i) = v;
            }
            if (chunk == chunks - 1 && tail0 + lane < (size_t)S) orow[tail0 + lane] = ar[tail0 + lane] * sv + b;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long long i = (long long)chunk * 256 + j * 64 + lane;
                if (i < S) orow[i] = ar[i] * sv + b;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// the excitation MLP: one workgroup per sample, z / h (forward) and dp2 / dh (backward) in LDS
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void se_excite_fwd_kernel(const float* __restrict__ rowsum, int C, int A, int Cg, int Hd,
                                                            float inv_as, const float* __restrict__ w1,
                                                            const float* __restrict__ b1, const float* __restrict__ w2,
                                                            const float* __restrict__ b2, float* __restrict__ z,
                                                            float* __restrict__ h, float* __restrict__ s) {
    __shared__ float zs[SELD_SE_MAX_GATED];
    __shared__ float hs[SELD_SE_MAX_HIDDEN];
    const size_t n = blockIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    // z: the A component sums of a gated channel folded k = 0, 1, ..., then the mean
    for (int g = threadIdx.x; g < Cg; g += 256) {
        float acc = rowsum[n * C + g];
        for (int k = 1; k < A; ++k) acc += rowsum[n * C + (size_t)k * Cg + g];
        const float zv = acc * inv_as;
        zs[g] = zv;
        z[n * Cg + g] = zv;
    }
    __syncthreads();
    // h = relu(W1 z + b1): one wave per row of W1, lanes stride the row
    for (int r = wave; r < Hd; r += 4) {
        float acc = 0.f;
        for (int g = lane; g < Cg; g += 64) acc += w1[(size_t)r * Cg + g] * zs[g];
        acc = wave_sum(acc) + b1[r];
        const float hv = acc > 0.f ? acc : 0.f;
        if (lane == 0) {
            hs[r] = hv;
            h[n * Hd + r] = hv;
        }
    }
    __syncthreads();
    // s = sigmoid(W2 h + b2): one wave per row of W2
    for (int g = wave; g < Cg; g += 4) {
        float acc = 0.f;
        for (int r = lane; r < Hd; r += 64) acc += w2[(size_t)g * Hd + r] * hs[r];
        acc = wave_sum(acc) + b2[g];
        if (lane == 0) s[n * Cg + g] = 1.0f / (1.0f + expf(-acc));
    }
}

__global__ __launch_bounds__(256) void se_excite_bwd_kernel(const float* __restrict__ q, int C, int A, int Cg, int Hd,
                                                            const float* __restrict__ w1, const float* __restrict__ w2,
                                                            const float* __restrict__ h, const float* __restrict__ s,
                                                            float* __restrict__ dp2, float* __restrict__ dh,
                                                            float* __restrict__ dz) {
    __shared__ float dps[SELD_SE_MAX_GATED];
    __shared__ float dhs[SELD_SE_MAX_HIDDEN];
    const size_t n = blockIdx.x;
    for (int g = threadIdx.x; g < Cg; g += 256) {
        float acc = q[n * C + g];
        for (int k = 1; k < A; ++k) acc += q[n * C + (size_t)k * Cg + g];
        const float sv = s[n * Cg + g];
        const float d = (acc * sv) * (1.0f - sv);
        dps[g] = d;
        dp2[n * Cg + g] = d;
    }
    __syncthreads();
    // dh = (W2^T dp2) [h > 0]: one thread per column of W2 (neighbouring threads read neighbouring floats), g = 0, 1, ...
    for (int r = threadIdx.x; r < Hd; r += 256) {
        float acc = 0.f;
        for (int g = 0; g < Cg; ++g) acc += w2[(size_t)g * Hd + r] * dps[g];
        const float v = h[n * Hd + r] > 0.f ? acc : 0.f;
        dhs[r] = v;
        dh[n * Hd + r] = v;
    }
    __syncthreads();
    // dz = W1^T dh: one thread per column of W1, r = 0, 1, ...
    for (int g = threadIdx.x; g < Cg; g += 256) {
        float acc = 0.f;
        for (int r = 0; r < Hd; ++r) acc += w1[(size_t)r * Cg + g] * dhs[r];
        dz[n * Cg + g] = acc;
    }
}

// [dW1 (Hd, Cg) | db1 (Hd) | dW2 (Cg, Hd) | db2 (Cg)]: one thread per element, the batch summed n = 0, 1, ... in order
__global__ __launch_bounds__(256) void se_param_grads_kernel(int N, int Cg, int Hd, const float* __restrict__ z,
                                                             const float* __restrict__ h, const float* __restrict__ dp2,
                                                             const float* __restrict__ dh, float* __restrict__ dw1,
                                                             float* __restrict__ db1, float* __restrict__ dw2,
                                                             float* __restrict__ db2, int accumulate) {
    const long long HC = (long long)Hd * Cg;
    const long long total = 2 * HC + Hd + Cg;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        float acc = 0.f;
        float* dst;
        if (i < HC) {                       // dW1[r, g] = sum_n dh[n, r] z[n, g]
            const int r = (int)(i / Cg), g = (int)(i - (long long)r * Cg);
            for (int n = 0; n < N; ++n) acc += dh[(size_t)n * Hd + r] * z[(size_t)n * Cg + g];
            dst = dw1 + i;
        } else if (i < HC + Hd) {           // db1[r] = sum_n dh[n, r]
            const int r = (int)(i - HC);
            for (int n = 0; n < N; ++n) acc += dh[(size_t)n * Hd + r];
            dst = db1 + r;
        } else if (i < 2 * HC + Hd) {       // dW2[g, r] = sum_n dp2[n, g] h[n, r]
            const long long j = i - HC - Hd;
            const int g = (int)(j / Hd), r = (int)(j - (long long)g * Hd);
            for (int n = 0; n < N; ++n) acc += dp2[(size_t)n * Cg + g] * h[(size_t)n * Hd + r];
            dst = dw2 + j;
        } else {                            // db2[g] = sum_n dp2[n, g]
            const int g = (int)(i - 2 * HC - Hd);
            for (int n = 0; n < N; ++n) acc += dp2[(size_t)n * Cg + g];
            dst = db2 + g;
        }
        *dst = accumulate ? *dst + acc : acc;
    }
}

}  // namespace seld

using namespace seld;
#define ST(s) ((hipStream_t)(s))

static inline bool se_block_form(int S) { return S >= SELD_SE_BLOCK_MIN_S; }
static inline unsigned se_grid(long long rows, bool block) {
    const long long b = block ? rows : (rows + 3) / 4;
    return (unsigned)(b > (1LL << 20) ? (1LL << 20) : b);        // the kernels stride over the rows beyond
}
// every tensor of the call at the same offset from a 16-byte boundary: then so is every row of each
static inline bool se_same_phase(const void* a, const void* b) { return (((uintptr_t)a ^ (uintptr_t)b) & 15u) == 0; }
static inline float se_inv_as(int A, int S) { return (float)(1.0 / ((double)A * (double)S)); }
static inline bool se_dims_bad(int N, int C, int S, int A) {
    return N <= 0 || C <= 0 || S <= 0 || (A != 1 && A != 4 && A != 8) || C % A != 0;
}

#define SE_DISPATCH(kernel, vec, block, grid, ...)                                                            \
    do {                                                                                                      \
        if (vec && block) hipLaunchKernelGGL((kernel<true, true>), grid, dim3(256), 0, __VA_ARGS__);          \
        else if (vec) hipLaunchKernelGGL((kernel<true, false>), grid, dim3(256), 0, __VA_ARGS__);             \
        else if (block) hipLaunchKernelGGL((kernel<false, true>), grid, dim3(256), 0, __VA_ARGS__);           \
        else hipLaunchKernelGGL((kernel<false, false>), grid, dim3(256), 0, __VA_ARGS__);                     \
    } while (0)

// chunks of a row for se_scale_kernel: 64 groups of four cover groups <= S / 4 (x4), 256 elements (x1)
static inline int se_chunks(int S, bool vec) { return vec ? (S / 4 + 63) / 64 + (S < 4) : (S + 255) / 256; }
static int se_launch_scale(const float* a, long long rows, int A, int Cg, int S, const float* s, const float* add,
                           float inv_as, float* out, hipStream_t stream) {
    const bool vec = se_same_phase(a, out);
    const int chunks = se_chunks(S, vec), log2A = A == 8 ? 3 : A == 4 ? 2 : 0;
    const long long items = rows * chunks, blocks = (items + 3) / 4;
    if (items + 4LL * 8192 >= (1LL << 32)) return SELD_EUNSUPPORTED;    // the kernel's strided index stays below 2^32
    const dim3 grid((unsigned)(blocks > 8192 ? 8192 : blocks));         // the kernel strides over the items beyond
    if (vec) hipLaunchKernelGGL(se_scale_kernel<true>, grid, dim3(256), 0, stream, a, (unsigned)items, log2A, Cg, S, chunks, s, add, inv_as, out);
    else hipLaunchKernelGGL(se_scale_kernel<false>, grid, dim3(256), 0, stream, a, (unsigned)items, log2A, Cg, S, chunks, s, add, inv_as, out);
    return check_launch();
}

extern "C" int seld_se_squeeze(const float* x, int64_t rows, int32_t S, float* rowsum, void* stream) {
    if (!x || !rowsum || rows <= 0 || S <= 0) return SELD_EINVAL;
    const bool block = se_block_form(S);
    SE_DISPATCH(se_squeeze_kernel, true, block, dim3(se_grid(rows, block)), ST(stream), x, (long long)rows, S, rowsum);
    return check_launch();
}

extern "C" int seld_se_bwd_reduce(const float* dy, const float* x, int64_t rows, int32_t S, float* q, void* stream) {
    if (!dy || !x || !q || rows <= 0 || S <= 0) return SELD_EINVAL;
    const bool block = se_block_form(S), vec = se_same_phase(dy, x);
    SE_DISPATCH(se_bwd_reduce_kernel, vec, block, dim3(se_grid(rows, block)), ST(stream), dy, x, (long long)rows, S, q);
    return check_launch();
}

extern "C" int seld_se_scale(const float* x, int32_t N, int32_t C, int32_t S, int32_t A, const float* s, float* y,
                             void* stream) {
    if (!x || !s || !y || se_dims_bad(N, C, S, A)) return SELD_EINVAL;
    const long long rows = (long long)N * C;
    return se_launch_scale(x, rows, A, C / A, S, s, nullptr, 0.f, y, ST(stream));
}

extern "C" int seld_se_bwd_apply(const float* dy, int32_t N, int32_t C, int32_t S, int32_t A, const float* s,
                                 const float* dz, float* dx, void* stream) {
    if (!dy || !s || !dz || !dx || se_dims_bad(N, C, S, A)) return SELD_EINVAL;
    const long long rows = (long long)N * C;
    return se_launch_scale(dy, rows, A, C / A, S, s, dz, se_inv_as(A, S), dx, ST(stream));
}

extern "C" int seld_se_excite_fwd(const float* rowsum, int32_t N, int32_t C, int32_t S, int32_t A, int32_t Hd,
                                  const float* w1, const float* b1, const float* w2, const float* b2, float* z, float* h,
                                  float* s, void* stream) {
    if (!rowsum || !w1 || !b1 || !w2 || !b2 || !z || !h || !s || Hd <= 0 || se_dims_bad(N, C, S, A)) return SELD_EINVAL;
    if (C / A > SELD_SE_MAX_GATED || Hd > SELD_SE_MAX_HIDDEN) return SELD_EUNSUPPORTED;
    hipLaunchKernelGGL(se_excite_fwd_kernel, dim3(N), dim3(256), 0, ST(stream), rowsum, C, A, C / A, Hd, se_inv_as(A, S), w1,
                       b1, w2, b2, z, h, s);
    return check_launch();
}

extern "C" int seld_se_excite_bwd(const float* q, int32_t N, int32_t C, int32_t A, int32_t Hd, const float* w1,
                                  const float* w2, const float* z, const float* h, const float* s, float* dp2, float* dh,
                                  float* dz, float* dw1, float* db1, float* dw2, float* db2, int32_t accumulate,
                                  void* stream) {
    if (!q || !w1 || !w2 || !z || !h || !s || !dp2 || !dh || !dz || !dw1 || !db1 || !dw2 || !db2 || Hd <= 0 ||
        se_dims_bad(N, C, 1, A))
        return SELD_EINVAL;
    const int Cg = C / A;
    if (Cg > SELD_SE_MAX_GATED || Hd > SELD_SE_MAX_HIDDEN) return SELD_EUNSUPPORTED;
    hipLaunchKernelGGL(se_excite_bwd_kernel, dim3(N), dim3(256), 0, ST(stream), q, C, A, Cg, Hd, w1, w2, h, s, dp2, dh, dz);
    const long long total = 2LL * Hd * Cg + Hd + Cg;
    hipLaunchKernelGGL(se_param_grads_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ST(stream), N, Cg, Hd, z,
                       h, dp2, dh, dw1, db1, dw2, db2, accumulate);
    return check_launch();
}

// Which form a streaming entry point launches, from the same selection functions the entry points use.
extern "C" int seld_se_kernel_label(int32_t op, int32_t S, int32_t same_phase, char* buf, int32_t buflen) {
    static const char* const names[] = {"se_squeeze", "se_scale", "se_bwd_reduce", "se_bwd_apply"};
    if (op < 0 || op > SELD_SE_BWD_APPLY || S <= 0 || !buf || buflen < 48) return SELD_EINVAL;
    const bool vec = op == SELD_SE_SQUEEZE || same_phase;
    const bool sums = op == SELD_SE_SQUEEZE || op == SELD_SE_BWD_REDUCE;
    snprintf(buf, buflen, "%s_%s_kernel[x%d]", names[op], !sums ? "chunk" : se_block_form(S) ? "block" : "row", vec ? 4 : 1);
    return SELD_OK;
}
