// What norm.hip, elementwise.hip and train_step.hip share: the activation and its derivative, the launch grids of the
// grid-stride kernels, the stream cast.
#pragma once
#include "common.h"

namespace seld {

__device__ __forceinline__ float act_apply(float z, int act) {
    switch (act) {
        case SELD_ACT_RELU: return z > 0.f ? z : 0.f;
        case SELD_ACT_TANH: return tanhf(z);
        case SELD_ACT_SIGMOID: return 1.0f / (1.0f + expf(-z));
        default: return z;
    }
}
// derivative expressed through the OUTPUT y = act(z)
__device__ __forceinline__ float act_grad_from_y(float y, int act) {
    switch (act) {
        case SELD_ACT_RELU: return y > 0.f ? 1.f : 0.f;
        case SELD_ACT_TANH: return 1.f - y * y;
        case SELD_ACT_SIGMOID: return y * (1.f - y);
        default: return 1.f;
    }
}

// one wave per row, 4 rows per block
static inline unsigned row_grid(long long rows) {
    long long b = (rows + 3) / 4;
    return (unsigned)(b < 1 ? 1 : (b > 65535 ? 65535 : b));
}

static inline unsigned grid_for(long long work_items, int per_block = 256, int cap = 8192) {
    long long b = (work_items + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (unsigned)b;
}

}  // namespace seld

#define ST(s) ((hipStream_t)(s))
