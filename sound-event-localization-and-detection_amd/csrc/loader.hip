// Device-resident epoch loader: the minibatch of a training step is gathered out of the resident dataset by a launch
// that reads WHICH batch from device memory, so the launch can be recorded once in a HIP graph and fetch the next batch
// at every replay (train.ResidentLoader, train.GraphedTrainStep).
//
//   seld_gather_rows      out[b, :] = all[index[cursor * stride + start + b], :] for the predictors and the targets
//   seld_epoch_step_end   running mean of the loss, cursor += 1 (the last launch of a step)
//
// The gather is an HBM-bound copy (config 3: 2 MB per predictor row, 67 MB per batch): a row is spread over many
// workgroups in tiles of 16 KB (256 lanes x 4 x 16 bytes, all four loads issued before the first store), the grid is
// capped near 2048 workgroups and strides over the tiles beyond that.  The loads of `cursor` and `index` depend on the
// workgroup's coordinates only: the compiler keeps them on the scalar unit.  No LDS.
#include "common.h"

namespace seld {

constexpr int GATHER_THREADS = 256;
constexpr int GATHER_VEC = 4;                                           // 16-byte accesses per lane and tile
constexpr long long GATHER_TILE = (long long)GATHER_THREADS * GATHER_VEC * 4;   // floats per tile
constexpr int GATHER_MAX_BLOCKS = 2048;

struct GatherSide {
    const float* all;   // (n_rows, row)
    float* out;         // (B, row)
    long long row;
};

// `len` <= GATHER_TILE floats from s to d (zeros when !valid; s is then not read).  16-byte accesses over the part where
// source and destination are 16-byte aligned TOGETHER, single floats before and behind it; when the two are aligned
// differently (a row length that is no multiple of 4 puts every other row there) the whole tile moves float by float.
__device__ __forceinline__ void gather_tile(const float* __restrict__ s, float* __restrict__ d, int len, bool valid) {
    const int tid = threadIdx.x;
    const uintptr_t da = (uintptr_t)d, sa = valid ? (uintptr_t)s : (uintptr_t)d;
    if ((da ^ sa) & 15) {
        for (int i = tid; i < len; i += GATHER_THREADS) d[i] = s[i];
        return;
    }
    int head = (int)(((16 - (da & 15)) & 15) >> 2);
    if (head > len) head = len;
    if (tid < head) d[tid] = valid ? s[tid] : 0.f;
    const int nv = (len - head) >> 2;
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(s + head);
    float4* __restrict__ d4 = reinterpret_cast<float4*>(d + head);
    float4 v[GATHER_VEC];
#pragma unroll
    for (int k = 0; k < GATHER_VEC; ++k) {
        const int i = tid + k * GATHER_THREADS;
        v[k] = (valid && i < nv) ? s4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < GATHER_VEC; ++k) {
        const int i = tid + k * GATHER_THREADS;
        if (i < nv) d4[i] = v[k];
    }
    const int done = head + 4 * nv;
    if (tid < len - done) d[done + tid] = valid ? s[done + tid] : 0.f;
}

// grid (gx + gy, count): workgroups [0, gx) of a row copy the predictors, the rest the targets
__global__ __launch_bounds__(GATHER_THREADS) void gather_rows_kernel(GatherSide x, GatherSide y, int gx,
                                                                     const int64_t* __restrict__ index, long long n_index,
                                                                     long long n_rows, const int32_t* __restrict__ cursor,
                                                                     long long stride, long long start) {
    const int b = blockIdx.y;
    const bool is_y = (int)blockIdx.x >= gx;
    const GatherSide sd = is_y ? y : x;
    const int first = is_y ? (int)blockIdx.x - gx : (int)blockIdx.x;
    const int step = is_y ? (int)gridDim.x - gx : gx;
    const long long p = start + b + (cursor ? (long long)cursor[0] * stride : 0);
    long long r = -1;
    if (p >= 0 && p < n_index) r = index[p];
    const bool valid = r >= 0 && r < n_rows;        // anything else: the row is zero-filled, nothing is read
    float* dst = sd.out + (long long)b * sd.row;
    const float* src = valid ? sd.all + r * sd.row : dst;
    for (long long off = (long long)first * GATHER_TILE; off < sd.row; off += (long long)step * GATHER_TILE) {
        const long long left = sd.row - off;
        gather_tile(src + off, dst + off, (int)(left < GATHER_TILE ? left : GATHER_TILE), valid);
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

extern "C" int seld_gather_rows(const float* x_all, int64_t row_x, float* out_x, const float* y_all, int64_t row_y,
                                float* out_y, const int64_t* index, int64_t n_index, int64_t n_rows, const int32_t* cursor,
                                int64_t cursor_stride, int64_t start, int32_t B, int32_t count, void* stream) {
    const bool has_x = x_all || out_x, has_y = y_all || out_y;
    if (!index || n_index <= 0 || n_rows <= 0 || B <= 0 || count <= 0 || count > B || count > 65535) return SELD_EINVAL;
    if (!has_x && !has_y) return SELD_EINVAL;
    if (has_x && (!x_all || !out_x || row_x <= 0)) return SELD_EINVAL;
    if (has_y && (!y_all || !out_y || row_y <= 0)) return SELD_EINVAL;
    if (cursor && cursor_stride < 0) return SELD_EINVAL;
    const long long cap = GATHER_MAX_BLOCKS / count > 0 ? GATHER_MAX_BLOCKS / count : 1;
    const long long tx = has_x ? (row_x + GATHER_TILE - 1) / GATHER_TILE : 0, ty = has_y ? (row_y + GATHER_TILE - 1) / GATHER_TILE : 0;
    const int gx = (int)(tx < cap ? tx : cap), gy = (int)(ty < cap ? ty : cap);
    const GatherSide x{x_all, out_x, has_x ? (long long)row_x : 0}, y{y_all, out_y, has_y ? (long long)row_y : 0};
    hipLaunchKernelGGL(gather_rows_kernel, dim3(gx + gy, count), dim3(GATHER_THREADS), 0, (hipStream_t)stream, x, y, gx, index,
                       (long long)n_index, (long long)n_rows, cursor, (long long)cursor_stride, (long long)start);
    return check_launch();
}

extern "C" int seld_epoch_step_end(const float* loss, float* mean, int32_t* cursor, void* stream) {
    if (!loss || !mean || !cursor) return SELD_EINVAL;
    hipLaunchKernelGGL(epoch_step_end_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, loss, mean, cursor);
    return check_launch();
}
