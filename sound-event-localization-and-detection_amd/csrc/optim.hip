// The optimiser's extras, for gfx950: the global gradient norm with its clip coefficient (one launch, nothing read back),
// and Adam over the flat buffers with the coefficient read from device memory, decoupled (AdamW) decay and an
// exponential moving average of the weights folded into the update.  adam_kernel / adam_state_kernel (train_step.hip)
// stay what a step without extras launches.
#include "nn_common.h"

namespace seld {

// ------------------------------------------------------------------------------------------
// ||g * grad_scale||_2 and torch.nn.utils.clip_grad_norm_'s coefficient (include/seld_hip.h: seld_grad_norm)
// ------------------------------------------------------------------------------------------
constexpr int NORM_BLOCKS = 256;            // the grid is min(ceil(n / 256), NORM_BLOCKS): a function of n alone
__device__ double g_norm_part[NORM_BLOCKS];
__device__ unsigned g_norm_ticket;          // zero at module load, handed back zero by every launch

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the four wave sums of a 256-thread workgroup, added in a fixed order; every thread gets the total
__device__ __forceinline__ double block_sum_f64(double v, double (&red)[4]) {
    const double s = wave_sum_f64(v);
    __syncthreads();            // red may still be read from the previous call
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// Squares and sums in fp64: the square of an fp32 value is exact there, 1e30^2 is finite and a sum of n positive terms
// is off by at most n 2^-53 relative, so the one rounding that counts is the cast of the square root to fp32.
// Thread, wave and workgroup partials, then -- as loss_ticketed_sums does it, with a ticket and partials of its own --
// the workgroup that draws the last ticket adds the workgroup sums in a fixed order: no float atomics, the same bits
// from run to run.  At a few MB the launch is a chain of latencies, not of bytes, and three things keep the chain short.
// A thread's elements are taken NORM_UNROLL at a time, the loads of a round independent of one another and issued
// together (an element past the end counts as +0, which changes no sum).  A workgroup hands its sum over as ONE
// write-through (agent-scope) 8-byte store, waited for before it draws its ticket: the payload is that store alone,
// so no release fence is needed, and a fence would write back every line the backward pass left dirty in the XCD's L2,
// once per workgroup.  And there are only NORM_BLOCKS tickets on the one counter, which the last workgroup, after its
// acquire, reads with one load per thread instead of one wave walking them.
constexpr int NORM_UNROLL = 16;
__global__ __launch_bounds__(256) void grad_norm_kernel(const float* __restrict__ g, long long n, float gscale,
                                                        float max_norm, float* __restrict__ clip) {
    __shared__ double red[4];
    __shared__ int last;
    const long long stride = (long long)gridDim.x * blockDim.x;
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += NORM_UNROLL * stride) {
        float x[NORM_UNROLL];
#pragma unroll
        for (int k = 0; k < NORM_UNROLL; ++k) {
            // every load is unconditional (past the end it re-reads element i and the value is dropped): behind a
            // branch each load would be waited for before the next is issued
            const long long j = i + k * stride;
            const float gj = g[j < n ? j : i];
            x[k] = j < n ? gj * gscale : 0.f;           // the fp32 product adam_kernel forms
        }
#pragma unroll
        for (int k = 0; k < NORM_UNROLL; ++k) acc += (double)x[k] * (double)x[k];
    }
    const double block = block_sum_f64(acc, red);
    if (threadIdx.x == 0) {
        __hip_atomic_store(&g_norm_part[blockIdx.x], block, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // the store has landed before the ticket is drawn
        last = __hip_atomic_fetch_add(&g_norm_ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
        if (last) {
            // the acquire for the whole workgroup: this lane's fence and wait, then the barrier below, then the loads
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (!last) return;
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < NORM_BLOCKS / 256; ++k) {
        const int b = threadIdx.x + 256 * k;
        // agent-scope loads: served by L2, never by a line this CU's L1 kept from an earlier launch; unconditional, as above
        const double part = __hip_atomic_load(&g_norm_part[b < (int)gridDim.x ? b : 0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        t += b < (int)gridDim.x ? part : 0.0;
    }
    t = block_sum_f64(t, red);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(t);
        // clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max = 1).  An infinite norm gives 0, a NaN norm NaN
        // (the comparison is false), as torch.clamp does; no step is skipped here
        float c = max_norm / (norm + 1e-6f);
        c = c > 1.f ? 1.f : c;
        clip[0] = norm;
        clip[1] = c;
        clip[2] = fmaxf(clip[2], norm);
        clip[3] += c < 1.f ? 1.f : 0.f;
        g_norm_ticket = 0;      // ready for the next launch (launches on one device must not overlap)
    }
}

// ------------------------------------------------------------------------------------------
// Adam with the extras.  One body; the two kernels differ in where step and lr come from, as adam_kernel and
// adam_state_kernel do.  With clip == NULL, ema == NULL and decoupled == 0 the expressions are adam_kernel's.
// ------------------------------------------------------------------------------------------
struct AdamEx {
    float b1, b2, eps, wd;
    int decoupled;
    float gscale;
    const float* clip;          // nullable: clip[1] is the coefficient seld_grad_norm left
    float* ema;                 // nullable
    float ema_decay;
};

__device__ __forceinline__ void adam_ex_elements(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                 float* __restrict__ v, long long n, float lr, float step, const AdamEx a) {
    // fp contraction is off and the two fused operations are written out: every product and sum below rounds once, in
    // the places where adam_kernel as compiled rounds (its moments are product, product, sum; its update is one fma).
    // Left to the compiler, the branches around them change which pairs it fuses, and "extras off" stops being
    // adam_kernel bit for bit.
#pragma clang fp contract(off)
    const float b1 = a.b1, b2 = a.b2, eps = a.eps, wd = a.wd, gscale = a.gscale;
    // bias corrections ON THE DEVICE, with the expressions of adam_kernel
    const float bc1 = 1.0f - powf(b1, step);
    const float bc2_sqrt = sqrtf(1.0f - powf(b2, step));
    const float c = a.clip ? a.clip[1] : 1.f;
    const float keep = 1.f - lr * wd;                                       // torch.optim.AdamW: p *= 1 - lr * wd
    const float d = fminf(a.ema_decay, (1.f + step) / (10.f + step));       // the EMA's warm-up: 2/11, 3/12, ... up to the decay
    const float omd = 1.f - d;
    float* __restrict__ ema = a.ema;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float grad = g[i] * gscale;
        if (a.clip) grad *= c;
        float pv = p[i];
        if (a.decoupled) pv *= keep;
        else if (wd != 0.f) grad = fmaf(wd, pv, grad);       // one rounding: g and wd * p may cancel
        const float mi = b1 * m[i] + (1.f - b1) * grad;
        const float vi = b2 * v[i] + (1.f - b2) * grad * grad;
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        const float pn = fmaf(-(lr / bc1), mi / denom, pv);
        p[i] = pn;
        if (ema) {
            // d e + (1 - d) p written from e's side: an average that equals the weight stays on it exactly
            const float e = ema[i];
            ema[i] = e + omd * (pn - e);
        }
    }
}

__global__ __launch_bounds__(256) void adam_ex_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                      float* __restrict__ m, float* __restrict__ v, long long n, float lr,
                                                      float step, AdamEx a) {
    adam_ex_elements(p, g, m, v, n, lr, step, a);
}

// step and lr from the device-resident step state, and the end of the step (state[0] += state[3]), as adam_state_kernel
__global__ __launch_bounds__(256) void adam_ex_state_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                            float* __restrict__ m, float* __restrict__ v, long long n,
                                                            AdamEx a, uint64_t* __restrict__ state) {
    if (blockIdx.x == 0 && threadIdx.x == 0) state[0] += state[3];
    const float step = (float)state[1];
    const float lr = __uint_as_float((unsigned)state[2]);
    adam_ex_elements(p, g, m, v, n, lr, step, a);
}

static bool adam_ex_args_ok(const float* param, const float* grad, const float* exp_avg, const float* exp_avg_sq,
                            const float* ema, int64_t n, float ema_decay) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n < 0) return false;
    return !ema || (ema_decay >= 0.f && ema_decay < 1.f);
}

}  // namespace seld

using namespace seld;

extern "C" int seld_grad_norm(const float* grad, int64_t n, float grad_scale, float max_norm, float* clip, void* stream) {
    if ((n > 0 && !grad) || !clip || n < 0 || !(max_norm > 0.f)) return SELD_EINVAL;
    // n == 0 still launches (one workgroup): norm 0, coefficient 1
    hipLaunchKernelGGL(grad_norm_kernel, dim3(grid_for(n, 256, NORM_BLOCKS)), dim3(256), 0, ST(stream), grad, (long long)n,
                       grad_scale, max_norm, clip);
    return check_launch();
}

extern "C" int seld_adam_flat_ex(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                                 float lr, float beta1, float beta2, float eps, float weight_decay, int32_t decoupled,
                                 int32_t step, float grad_scale, const float* clip, float ema_decay, void* stream) {
    if (!adam_ex_args_ok(param, grad, exp_avg, exp_avg_sq, ema, n, ema_decay) || step < 1) return SELD_EINVAL;
    if (n == 0) return SELD_OK;
    const AdamEx a{beta1, beta2, eps, weight_decay, decoupled != 0, grad_scale, clip, ema, ema_decay};
    hipLaunchKernelGGL(adam_ex_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), param, grad, exp_avg, exp_avg_sq,
                       (long long)n, lr, (float)step, a);
    return check_launch();
}

extern "C" int seld_adam_flat_state_ex(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                                       int64_t n, float beta1, float beta2, float eps, float weight_decay,
                                       int32_t decoupled, float grad_scale, const float* clip, float ema_decay,
                                       uint64_t* state, void* stream) {
    if (!adam_ex_args_ok(param, grad, exp_avg, exp_avg_sq, ema, n, ema_decay) || !state) return SELD_EINVAL;
    // n == 0 still launches (one workgroup): the end of the step moves the Philox base, as seld_adam_flat_state
    const AdamEx a{beta1, beta2, eps, weight_decay, decoupled != 0, grad_scale, clip, ema, ema_decay};
    hipLaunchKernelGGL(adam_ex_state_kernel, dim3(grid_for(n)), dim3(256), 0, ST(stream), param, grad, exp_avg, exp_avg_sq,
                       (long long)n, a, state);
    return check_launch();
}
