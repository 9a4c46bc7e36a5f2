// Target encoding and segmentation on the device: the label path of the preparation half.
//
// Replaces
//   csv_to_matrix_task2   utility_functions.py:219-267   (the fill loop: events -> dense [activity | location] target)
//   segment_waveforms     utility_functions.py:272-299   (cut + zero-pad, no overlap)
//   segment_task2         utility_functions.py:302-342   (overlapping cut + zero-pad of features and target)
//
// encode: the inverse of decode.hip.  One workgroup per (recording, tile of ENC_TILE frames).  The recording's events
// (first, last, class) are staged in LDS; one thread per (frame, class) cell walks them IN EVENT ORDER and hands the
// k-th event that covers its frame slot k of its class, which is the reference's `pos = int(np.sum(cl[f][class_id]))`.
// A cell's thread writes all of the cell's elements, zeros included, into the tile's rows in LDS; the rows of a tile
// are one contiguous piece of the output and leave with 16-byte stores.  The coordinates are read from memory only
// for the slots that are filled.  The output has one writer per element and no atomics; the two counters (cells that
// overflow, invalid events) are folded per workgroup in LDS and added to memory once.
//
// segment: dst[s, r, j] = src[r, s * hop + j] or 0 past the end.  One thread per 16 bytes of dst, SEG_UNROLL of them in
// flight; the time-first layout is the same copy with rows = 1 and every extent multiplied by the row length.
#include "common.h"

namespace seld {

constexpr int ENC_THREADS = 256;
constexpr int ENC_TILE = 8;             // frames per workgroup: at most 8 * 256 * 8 = 16 KB of rows in LDS
constexpr int SEG_THREADS = 256;
constexpr int SEG_UNROLL = 4;           // 16-byte pieces per thread

__host__ __device__ inline size_t enc_tile_bytes(int row, int elem) { return (size_t)ENC_TILE * row * elem; }
// LDS: [counters 16 B | rows of the tile | first[cap] | last[cap] | class[cap] (1 byte each)]
__host__ __device__ inline size_t enc_lds_bytes(int row, int elem, int cap) {
    return 16 + enc_tile_bytes(row, elem) + (size_t)cap * 9;
}

template <typename T>
__global__ __launch_bounds__(ENC_THREADS) void encode_events_kernel(
    const int* __restrict__ first, const int* __restrict__ last, const int* __restrict__ cls, const double* __restrict__ xyz,
    const long long* __restrict__ rec_offsets, long long events, int cap, int tiles, int frames, int classes, int overlaps,
    int out_slots, double max_loc, int vec_ok, T* __restrict__ target, int* __restrict__ counters) {
    extern __shared__ __align__(16) unsigned char enc_lds[];
    const int row = 4 * classes * out_slots;
    int* cnt_s = reinterpret_cast<int*>(enc_lds);
    T* tile = reinterpret_cast<T*>(enc_lds + 16);
    int* ev_first = reinterpret_cast<int*>(enc_lds + 16 + enc_tile_bytes(row, (int)sizeof(T)));
    int* ev_last = ev_first + cap;
    unsigned char* ev_cls = reinterpret_cast<unsigned char*>(ev_last + cap);

    const int tid = threadIdx.x;
    const long long r = blockIdx.x / tiles;
    const int t = blockIdx.x % tiles;
    if (tid < 2) cnt_s[tid] = 0;

    // the recording's events, clamped so that no index leaves [0, events) whatever the offsets hold
    const long long o0 = rec_offsets[r], o1 = rec_offsets[r + 1];
    const long long e0 = min(max(o0, 0ll), events);
    const long long e1 = min(max(o1, e0), events);
    const int n = (int)min(e1 - e0, (long long)cap);
    int bad = (tid == 0) ? (int)(e0 != o0) + (int)(e1 != o1) + (int)(e1 - e0 > cap) : 0;
    for (int i = tid; i < n; i += ENC_THREADS) {
        const int a = first[e0 + i], b = last[e0 + i], c = cls[e0 + i];
        const bool ok = (unsigned)c < (unsigned)classes && (b < a || (a >= 0 && b < frames));
        ev_first[i] = a;
        ev_last[i] = b;
        ev_cls[i] = ok ? (unsigned char)c : (unsigned char)255;      // classes <= 64: 255 matches no cell
        bad += !ok;
    }
    __syncthreads();

    const int f0 = t * ENC_TILE;
    const int nf = min(ENC_TILE, frames - f0);
    const int ncl = classes * out_slots;
    const T zero_loc = (T)(0.0 / max_loc);                           // the reference divides the whole array
    int over = 0;
    for (int cell = tid; cell < nf * classes; cell += ENC_THREADS) {
        const int fl = cell / classes, c = cell - fl * classes, f = f0 + fl;
        T* cl_p = tile + (size_t)fl * row + c * out_slots;
        T* loc_p = tile + (size_t)fl * row + ncl + 3 * c * out_slots;
        int pos = 0;
        for (int i = 0; i < n; ++i) {
            if ((int)ev_cls[i] == c && ev_first[i] <= f && f <= ev_last[i]) {
                if (pos < out_slots) {
                    const double* q = xyz + (size_t)(e0 + i) * 3;
                    cl_p[pos] = (T)1;
                    loc_p[3 * pos + 0] = (T)(q[0] / max_loc);
                    loc_p[3 * pos + 1] = (T)(q[1] / max_loc);
                    loc_p[3 * pos + 2] = (T)(q[2] / max_loc);
                }
                ++pos;
            }
        }
        over += pos > overlaps;
        for (int s = min(pos, out_slots); s < out_slots; ++s) {
            cl_p[s] = (T)0;
            loc_p[3 * s + 0] = zero_loc;
            loc_p[3 * s + 1] = zero_loc;
            loc_p[3 * s + 2] = zero_loc;
        }
    }
    if (over) atomicAdd(&cnt_s[0], over);
    if (bad && t == 0) atomicAdd(&cnt_s[1], bad);                    // a recording's events are judged once
    __syncthreads();

    // the tile's rows are contiguous in the output: full 16-byte stores (row is a multiple of 4 elements)
    T* dst = target + ((size_t)r * frames + f0) * row;
    const int total = nf * row;
    if (vec_ok) {
        constexpr int V = 16 / (int)sizeof(T);
        const uint4* s4 = reinterpret_cast<const uint4*>(tile);
        uint4* d4 = reinterpret_cast<uint4*>(dst);
        for (int i = tid; i < total / V; i += ENC_THREADS) d4[i] = s4[i];
    } else {
        for (int i = tid; i < total; i += ENC_THREADS) dst[i] = tile[i];
    }
    if (tid < 2 && cnt_s[tid] != 0) atomicAdd(&counters[tid], cnt_s[tid]);
}

// dst (segments, rows, seg_len) from src (rows, length).  V elements (16 bytes, or 1) per piece; VLOAD: the pieces of
// src are 16-byte aligned too (pointer, length and hop all multiples of V).
template <typename T, int V, bool VLOAD>
__global__ __launch_bounds__(SEG_THREADS) void segment_kernel(const T* __restrict__ src, long long rows, long long length,
                                                             long long seg_len, long long hop, long long segments,
                                                             T* __restrict__ dst) {
    typedef T vec_t __attribute__((ext_vector_type(V)));
    const long long vpr = seg_len / V;                               // pieces per row of a segment
    const long long m = rows * vpr;                                  // pieces per segment
    const bool narrow = m < (1ll << 31);
    for (long long s = blockIdx.y; s < segments; s += gridDim.y) {
        const long long t0 = s * hop;
        T* d = dst + (size_t)s * rows * seg_len;
        vec_t v[SEG_UNROLL];
        long long idx[SEG_UNROLL];
#pragma unroll
        for (int u = 0; u < SEG_UNROLL; ++u) {
            idx[u] = ((long long)blockIdx.x * SEG_UNROLL + u) * SEG_THREADS + threadIdx.x;
            if (idx[u] < m) {
                long long rr, jv;
                if (narrow) {
                    rr = (unsigned)idx[u] / (unsigned)vpr;
                    jv = (unsigned)idx[u] - (unsigned)rr * (unsigned)vpr;
                } else {
                    rr = idx[u] / vpr;
                    jv = idx[u] - rr * vpr;
                }
                const long long tt = t0 + jv * V;
                const T* p = src + (size_t)rr * length + tt;
                if (VLOAD && tt + V <= length) {
                    v[u] = *reinterpret_cast<const vec_t*>(p);
                } else {
#pragma unroll
                    for (int k = 0; k < V; ++k) v[u][k] = tt + k < length ? p[k] : (T)0;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < SEG_UNROLL; ++u)
            if (idx[u] < m) *reinterpret_cast<vec_t*>(d + (size_t)idx[u] * V) = v[u];
    }
}

template <typename T>
static int segment_launch(const T* src, long long rows, long long length, long long seg_len, long long hop, long long segments,
                          T* dst, hipStream_t stream) {
    constexpr int V = 16 / (int)sizeof(T);
    const bool vstore = seg_len % V == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
    const bool vload = vstore && length % V == 0 && hop % V == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
    const long long m = vstore ? rows * (seg_len / V) : rows * seg_len;
    const long long per_block = (long long)SEG_THREADS * SEG_UNROLL;
    const long long bx = (m + per_block - 1) / per_block;
    if (bx >= (1ll << 31)) return SELD_EUNSUPPORTED;
    const dim3 grid((unsigned)bx, (unsigned)min(segments, 65535ll)), block(SEG_THREADS);
    if (vload)
        hipLaunchKernelGGL((segment_kernel<T, V, true>), grid, block, 0, stream, src, rows, length, seg_len, hop, segments, dst);
    else if (vstore)
        hipLaunchKernelGGL((segment_kernel<T, V, false>), grid, block, 0, stream, src, rows, length, seg_len, hop, segments, dst);
    else
        hipLaunchKernelGGL((segment_kernel<T, 1, false>), grid, block, 0, stream, src, rows, length, seg_len, hop, segments, dst);
    return check_launch();
}

}  // namespace seld

using namespace seld;

extern "C" int seld_encode_events(const int32_t* first_frame, const int32_t* last_frame, const int32_t* cls, const double* xyz,
                                  const int64_t* rec_offsets, int64_t events, int32_t max_rec_events, int64_t recordings,
                                  int32_t frames, int32_t classes, int32_t overlaps, double max_loc_value, int32_t no_overlaps,
                                  int32_t dtype, void* target, int32_t* overflow, void* stream) {
    if (recordings <= 0 || frames <= 0 || classes <= 0 || overlaps <= 0 || events < 0) return SELD_EINVAL;
    if (max_rec_events < 0 || max_rec_events > events) return SELD_EINVAL;
    if (dtype != SELD_DECODE_F32 && dtype != SELD_DECODE_F64) return SELD_EINVAL;
    if (!rec_offsets || !target || !overflow) return SELD_EINVAL;
    if (events > 0 && (!first_frame || !last_frame || !cls || !xyz)) return SELD_EINVAL;
    if ((int64_t)classes * overlaps > 64) return SELD_EUNSUPPORTED;
    if (max_rec_events > SELD_ENCODE_MAX_EVENTS) return SELD_EUNSUPPORTED;
    const int tiles = (frames + ENC_TILE - 1) / ENC_TILE;
    if (recordings > (int64_t)0x7fffffff / tiles) return SELD_EUNSUPPORTED;
    const int out_slots = no_overlaps ? 1 : overlaps;
    const int row = 4 * classes * out_slots;
    const int elem = dtype == SELD_DECODE_F32 ? 4 : 8;
    const size_t lds = enc_lds_bytes(row, elem, max_rec_events);
    const int vec_ok = (reinterpret_cast<uintptr_t>(target) & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t me = hipMemsetAsync(overflow, 0, 2 * sizeof(int32_t), st);
    if (me != hipSuccess) {
        g_last_hip_error = (int)me;
        return SELD_ELAUNCH;
    }
    const dim3 grid((unsigned)(recordings * tiles)), block(ENC_THREADS);
    if (dtype == SELD_DECODE_F32)
        hipLaunchKernelGGL(encode_events_kernel<float>, grid, block, lds, st, first_frame, last_frame, cls, xyz,
                           reinterpret_cast<const long long*>(rec_offsets), (long long)events, (int)max_rec_events, tiles, frames,
                           classes, overlaps, out_slots, max_loc_value, vec_ok, (float*)target, overflow);
    else
        hipLaunchKernelGGL(encode_events_kernel<double>, grid, block, lds, st, first_frame, last_frame, cls, xyz,
                           reinterpret_cast<const long long*>(rec_offsets), (long long)events, (int)max_rec_events, tiles, frames,
                           classes, overlaps, out_slots, max_loc_value, vec_ok, (double*)target, overflow);
    return check_launch();
}

extern "C" int seld_segment(const void* src, int32_t dtype, int32_t layout, int64_t rows, int64_t length, int64_t seg_len,
                            int64_t hop, int64_t segments, void* dst, void* stream) {
    if (!src || !dst || rows <= 0 || length <= 0 || seg_len <= 0 || hop < 1 || segments <= 0) return SELD_EINVAL;
    if (dtype != SELD_DECODE_F32 && dtype != SELD_DECODE_F64) return SELD_EINVAL;
    if (layout != SELD_SEGMENT_TIME_LAST && layout != SELD_SEGMENT_TIME_FIRST) return SELD_EINVAL;
    const __int128 lim = (__int128)1 << 46;
    if ((__int128)rows * length >= lim || (__int128)rows * seg_len >= lim || (__int128)segments * hop >= lim ||
        (__int128)segments * hop * rows >= ((__int128)1 << 62) || (__int128)segments * rows * seg_len >= ((__int128)1 << 60))
        return SELD_EUNSUPPORTED;
    if (layout == SELD_SEGMENT_TIME_FIRST) {                         // whole time steps are contiguous: one long row
        length *= rows;
        seg_len *= rows;
        hop *= rows;
        rows = 1;
    }
    if (dtype == SELD_DECODE_F32)
        return segment_launch<float>((const float*)src, rows, length, seg_len, hop, segments, (float*)dst, (hipStream_t)stream);
    return segment_launch<double>((const double*)src, rows, length, seg_len, hop, segments, (double*)dst, (hipStream_t)stream);
}
