// What every training step ends in, for gfx950: the SELD loss (plain and permutation-invariant) with its ticketed ordered
// sums, Adam over the flat parameter buffer, and the device-resident step state.
#include "nn_common.h"

namespace seld {

// ------------------------------------------------------------------------------------------
// loss = w_sed * mean BCE(sed, t_sed) + w_doa * mean MSE(doa, t_doa)     (train.py:186-204)
// ------------------------------------------------------------------------------------------
constexpr int LOSS_BLOCKS = 256;
__device__ float g_loss_part[LOSS_BLOCKS];
__device__ float g_loss_part_sed[LOSS_BLOCKS], g_loss_part_doa[LOSS_BLOCKS];       // the `parts` of loss_pit_kernel
__device__ unsigned g_loss_ticket;          // zero at module load, handed back zero by every launch

// The tail of both loss kernels, N sums at once.  Workgroup sums -> part[k]; the workgroup that draws the last ticket adds
// them in a fixed order and writes out[k] (out[0] always, the others where non-null): no zeroed accumulator (the host
// mirror used to launch a fill per step), the same bits for any grid.  Every thread of the workgroup calls it, last.
template <int N>
__device__ __forceinline__ void loss_ticketed_sums(const float (&acc)[N], float* const (&part)[N], float* const (&out)[N]) {
    __shared__ float red[N][4];
    __shared__ int last;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const float s = wave_sum(acc[k]);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) part[k][blockIdx.x] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
        __threadfence();
        last = atomicAdd(&g_loss_ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last || threadIdx.x >= 64) return;
    __threadfence();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if (k > 0 && !out[k]) continue;
        float t = 0.f;
        for (int b = threadIdx.x; b < (int)gridDim.x; b += 64) t += *(volatile float*)&part[k][b];
        t = wave_sum(t);
        if (threadIdx.x == 0) *out[k] = t;
    }
    // ready for the next evaluation (launches of the loss kernels on one device must not overlap)
    if (threadIdx.x == 0) g_loss_ticket = 0;
}

__global__ __launch_bounds__(256) void loss_kernel(const float* __restrict__ sed, const float* __restrict__ doa,
                                                   const float* __restrict__ target, long long rows, int n_sed, int n_doa,
                                                   float w_sed, float w_doa, float* __restrict__ loss,
                                                   float* __restrict__ dsed, float* __restrict__ ddoa) {
    const int ncol = n_sed + n_doa;
    const long long total = rows * ncol;
    const float inv_sed = 1.0f / (float)(rows * n_sed);
    const float inv_doa = 1.0f / (float)(rows * n_doa);
    float acc = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / ncol;
        const int c = (int)(i - r * ncol);
        const float t = target[i];
        if (c < n_sed) {
            const size_t o = (size_t)r * n_sed + c;
            const float s = sed[o];
            // torch.nn.BCELoss clamps the logs at -100
            const float l1 = fmaxf(logf(s), -100.f), l0 = fmaxf(logf(1.f - s), -100.f);
            acc += -(t * l1 + (1.f - t) * l0) * inv_sed * w_sed;
            if (dsed) dsed[o] = w_sed * inv_sed * (s - t) / fmaxf(s * (1.f - s), 1e-12f);
        } else {
            const size_t o = (size_t)r * n_doa + (c - n_sed);
            const float d = doa[o] - t;
            acc += d * d * inv_doa * w_doa;
            if (ddoa) ddoa[o] = w_doa * inv_doa * 2.f * d;
        }
    }
    const float accs[1] = {acc};
    float* const parts[1] = {g_loss_part};
    float* const outs[1] = {loss};
    loss_ticketed_sums<1>(accs, parts, outs);
}

// ------------------------------------------------------------------------------------------
// The same loss with, per (row, class) cell, the pairing of prediction slots with target slots that costs least
// (include/seld_hip.h: seld_loss_pit_fwd_bwd).  One thread per cell; a cell's O + 3 O prediction floats and O + 3 O target
// floats are contiguous runs and adjacent lanes take adjacent classes.  Everything of a cell lives in registers: the slot
// loops have the compile-time bound O and every array index is a constant after unrolling (0 scratch bytes).
// fp contraction is off in this kernel: a pair cost must have the same bits wherever it appears in a sum.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float pit_bce(float l1, float l0, float t) {
#pragma clang fp contract(off)
    return -(t * l1 + (1.f - t) * l0);
}
__device__ __forceinline__ float pit_sq(float p0, float p1, float p2, float t0, float t1, float t2) {
#pragma clang fp contract(off)
    const float d0 = p0 - t0, d1 = p1 - t1, d2 = p2 - t2;
    return (d0 * d0 + d1 * d1) + d2 * d2;
}
__device__ __forceinline__ float pit_pick(int j, float v0, float v1, float v2) { return j == 0 ? v0 : (j == 1 ? v1 : v2); }

#define PIT_TRY2(j0, j1, idx)                                                                                         \
    {                                                                                                                 \
        const float c_ = P[0][j0] + P[1][j1];                                                                         \
        if (c_ < best) { best = c_; bi = idx; s0 = j0; s1 = j1; }                                                     \
    }
#define PIT_TRY3(j0, j1, j2, idx)                                                                                     \
    {                                                                                                                 \
        const float c_ = (P[0][j0] + P[1][j1]) + P[2][j2];                                                            \
        if (c_ < best) { best = c_; bi = idx; s0 = j0; s1 = j1; s2 = j2; }                                            \
    }

template <int O>
__global__ __launch_bounds__(256) void loss_pit_kernel(const float* __restrict__ sed, const float* __restrict__ doa,
                                                       const float* __restrict__ target, long long rows, int classes,
                                                       float w_sed, float w_doa, float* __restrict__ loss,
                                                       float* __restrict__ dsed, float* __restrict__ ddoa,
                                                       int* __restrict__ perm, float* __restrict__ parts) {
#pragma clang fp contract(off)
    const int n_sed = classes * O, n_doa = 3 * n_sed, ncol = n_sed + n_doa;
    const long long cells = rows * classes;
    const float inv_sed = 1.0f / (float)(rows * n_sed);
    const float inv_doa = 1.0f / (float)(rows * n_doa);
    const float a = w_sed * inv_sed, b = w_doa * inv_doa;
    float acc = 0.f, acc_sed = 0.f, acc_doa = 0.f;
    for (long long cell = (long long)blockIdx.x * blockDim.x + threadIdx.x; cell < cells;
         cell += (long long)gridDim.x * blockDim.x) {
        const long long r = cell / classes;
        const int c = (int)(cell - r * classes);
        const size_t os = (size_t)cell * O, od = os * 3;                  // r * n_sed + c * O, r * n_doa + c * O * 3
        const float* ts_p = target + (size_t)r * ncol + (size_t)c * O;
        const float* td_p = target + (size_t)r * ncol + n_sed + (size_t)c * O * 3;
        float s[O], l1[O], l0[O], ts[O], d[O][3], td[O][3];
#pragma unroll
        for (int o = 0; o < O; ++o) {
            s[o] = sed[os + o];
            ts[o] = ts_p[o];
            // torch.nn.BCELoss clamps the logs at -100
            l1[o] = fmaxf(logf(s[o]), -100.f);
            l0[o] = fmaxf(logf(1.f - s[o]), -100.f);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                d[o][k] = doa[od + o * 3 + k];
                td[o][k] = td_p[o * 3 + k];
            }
        }
        float P[O][O];          // P[o][j]: prediction slot o against target slot j
#pragma unroll
        for (int o = 0; o < O; ++o)
#pragma unroll
            for (int j = 0; j < O; ++j)
                P[o][j] = a * pit_bce(l1[o], l0[o], ts[j]) + b * pit_sq(d[o][0], d[o][1], d[o][2], td[j][0], td[j][1], td[j][2]);
        // lexicographic order, from the identity, replaced on `<` only: ties go to the lowest index, a NaN cost never wins
        int bi = 0, s0 = 0, s1 = 1, s2 = 2;
        float best;
        if constexpr (O == 1) {
            best = P[0][0];
        } else if constexpr (O == 2) {
            best = P[0][0] + P[1][1];
            PIT_TRY2(1, 0, 1)
        } else {
            best = (P[0][0] + P[1][1]) + P[2][2];
            PIT_TRY3(0, 2, 1, 1)
            PIT_TRY3(1, 0, 2, 2)
            PIT_TRY3(1, 2, 0, 3)
            PIT_TRY3(2, 0, 1, 4)
            PIT_TRY3(2, 1, 0, 5)
        }
        (void)s2;
        // the chosen pairing's targets, then the plain loss's expressions on them
        float cs[O], cd[O];
#pragma unroll
        for (int o = 0; o < O; ++o) {
            const int j = o == 0 ? s0 : (o == 1 ? s1 : s2);
            float t, u0, u1, u2;
            if constexpr (O == 1) {
                t = ts[0]; u0 = td[0][0]; u1 = td[0][1]; u2 = td[0][2];
            } else {
                constexpr int L = O - 1;          // the last slot: pit_pick's third operand (O == 2: never picked)
                t = pit_pick(j, ts[0], ts[1], ts[L]);
                u0 = pit_pick(j, td[0][0], td[1][0], td[L][0]);
                u1 = pit_pick(j, td[0][1], td[1][1], td[L][1]);
                u2 = pit_pick(j, td[0][2], td[1][2], td[L][2]);
            }
            cs[o] = a * pit_bce(l1[o], l0[o], t);
            cd[o] = b * pit_sq(d[o][0], d[o][1], d[o][2], u0, u1, u2);
            if (dsed) dsed[os + o] = w_sed * inv_sed * (s[o] - t) / fmaxf(s[o] * (1.f - s[o]), 1e-12f);
            if (ddoa) {
                ddoa[od + o * 3 + 0] = w_doa * inv_doa * 2.f * (d[o][0] - u0);
                ddoa[od + o * 3 + 1] = w_doa * inv_doa * 2.f * (d[o][1] - u1);
                ddoa[od + o * 3 + 2] = w_doa * inv_doa * 2.f * (d[o][2] - u2);
            }
        }
        acc += best;
        if constexpr (O == 1) {
            acc_sed += cs[0];
            acc_doa += cd[0];
        } else if constexpr (O == 2) {
            acc_sed += cs[0] + cs[1];
            acc_doa += cd[0] + cd[1];
        } else {
            acc_sed += (cs[0] + cs[1]) + cs[2];
            acc_doa += (cd[0] + cd[1]) + cd[2];
        }
        if (perm) perm[cell] = bi;
    }
    const float accs[3] = {acc, acc_sed, acc_doa};
    float* const part[3] = {g_loss_part, g_loss_part_sed, g_loss_part_doa};
    float* const outs[3] = {loss, parts, parts ? parts + 1 : nullptr};
    loss_ticketed_sums<3>(accs, part, outs);
}
#undef PIT_TRY2
#undef PIT_TRY3

// ------------------------------------------------------------------------------------------
// Adam over a flat buffer (torch.optim.Adam, no amsgrad, L2 weight decay added to the grad)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, long long n, float lr,
                                                   float b1, float b2, float eps, float wd, float step,
                                                   float gscale) {
    // bias corrections ON THE DEVICE, with the expressions of adam_state_kernel: an eager step and a replayed one then
    // produce the same bits (the host's powf rounds differently now and then)
    const float bc1 = 1.0f - powf(b1, step);
    const float bc2_sqrt = sqrtf(1.0f - powf(b2, step));
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float grad = g[i] * gscale;
        const float pv = p[i];
        if (wd != 0.f) grad = fmaf(wd, pv, grad);       // one rounding: g and wd * p may cancel
        const float mi = b1 * m[i] + (1.f - b1) * grad;
        const float vi = b2 * v[i] + (1.f - b2) * grad * grad;
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        p[i] = pv - (lr / bc1) * (mi / denom);
    }
}

// The same update with the step number and the learning rate read from the device-resident step state
// (state[1] = 1-based step, low 32 bits of state[2] = lr as float bits): a launch recorded in a HIP graph then follows
// the optimiser's bias correction and the scheduler's learning rate from replay to replay.
__global__ __launch_bounds__(256) void adam_state_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v, long long n,
                                                         float b1, float b2, float eps, float wd, float gscale,
                                                         uint64_t* __restrict__ state) {
    // end of the step: the Philox base moves past this step's draws (nothing after Adam draws), so whatever is issued
    // next -- a replay or an eager launch with host offsets from 0 -- sees fresh counters
    if (blockIdx.x == 0 && threadIdx.x == 0) state[0] += state[3];
    const float step = (float)state[1];
    const float lr = __uint_as_float((unsigned)state[2]);
    const float bc1 = 1.0f - powf(b1, step);
    const float bc2_sqrt = sqrtf(1.0f - powf(b2, step));
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float grad = g[i] * gscale;
        const float pv = p[i];
        if (wd != 0.f) grad = fmaf(wd, pv, grad);       // one rounding: g and wd * p may cancel
        const float mi = b1 * m[i] + (1.f - b1) * grad;
        const float vi = b2 * v[i] + (1.f - b2) * grad * grad;
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        p[i] = pv - (lr / bc1) * (mi / denom);
    }
}

// Start of a training step: zero the flat gradient buffer (16-byte stores) and advance the optimiser step
//   state[1] += 1
// (the Philox base state[0] advances by state[3] = draws per step at the END of the step, in adam_state_kernel)
__global__ __launch_bounds__(256) void step_begin_kernel(float* __restrict__ g, long long n, uint64_t* __restrict__ state) {
    if (state && blockIdx.x == 0 && threadIdx.x == 0) state[1] += 1;
    const long long n4 = n >> 2;
    float4* g4 = reinterpret_cast<float4*>(g);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x)
        g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) g[(n4 << 2) + threadIdx.x] = 0.f;
}

}  // namespace seld

using namespace seld;

extern "C" int seld_loss_fwd_bwd(const float* sed, const float* doa, const float* target, int64_t rows, int32_t n_sed,
                                 int32_t n_doa, float w_sed, float w_doa, float* loss, float* dsed, float* ddoa,
                                 void* stream) {
    if (!sed || !doa || !target || !loss || rows <= 0 || n_sed <= 0 || n_doa <= 0) return SELD_EINVAL;
    hipLaunchKernelGGL(loss_kernel, dim3(grid_for(rows * (n_sed + n_doa), 256, LOSS_BLOCKS)), dim3(256), 0, ST(stream), sed, doa,
                       target, (long long)rows, n_sed, n_doa, w_sed, w_doa, loss, dsed, ddoa);
    return check_launch();
}

extern "C" int seld_loss_pit_fwd_bwd(const float* sed, const float* doa, const float* target, int64_t rows, int32_t classes,
                                     int32_t overlaps, float w_sed, float w_doa, float* loss, float* dsed, float* ddoa,
                                     int32_t* perm, float* parts, void* stream) {
    if (!sed || !doa || !target || !loss || rows <= 0 || classes <= 0 || overlaps <= 0) return SELD_EINVAL;
    if (overlaps > 3) return SELD_EUNSUPPORTED;
    const dim3 grid(grid_for(rows * classes, 256, LOSS_BLOCKS));
    auto kernel = overlaps == 1 ? loss_pit_kernel<1> : overlaps == 2 ? loss_pit_kernel<2> : loss_pit_kernel<3>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, ST(stream), sed, doa, target, (long long)rows, classes, w_sed, w_doa, loss,
                       dsed, ddoa, perm, parts);
    return check_launch();
}

extern "C" int seld_adam_flat(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                              float beta1, float beta2, float eps, float weight_decay, int32_t step, float grad_scale,
                              void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n < 0 || step < 1) return SELD_EINVAL;
    if (n == 0) return SELD_OK;
    hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), param, grad, exp_avg, exp_avg_sq,
                       (long long)n, lr, beta1, beta2, eps, weight_decay, (float)step, grad_scale);
    return check_launch();
}
extern "C" int seld_adam_flat_state(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                    float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                                    uint64_t* state, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !state || n < 0) return SELD_EINVAL;
    // n == 0 still launches (one workgroup): the end of the step moves the Philox base, as seld_step_begin(n == 0)
    // still advances the step number
    hipLaunchKernelGGL(adam_state_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), param, grad, exp_avg, exp_avg_sq,
                       (long long)n, beta1, beta2, eps, weight_decay, grad_scale, state);
    return check_launch();
}
extern "C" int seld_step_begin(float* flat_grad, int64_t n, uint64_t* state, void* stream) {
    if ((n > 0 && !flat_grad) || n < 0) return SELD_EINVAL;
    if (n > 0 && ((uintptr_t)flat_grad & 15)) return SELD_EINVAL;
    hipLaunchKernelGGL(step_begin_kernel, dim3(grid_for((n + 3) / 4, 256, 2048)), dim3(256), 0, ST(stream), flat_grad,
                       (long long)n, state);
    return check_launch();
}
