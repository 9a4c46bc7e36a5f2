// Event decoding on the device: the submission rows of a batch of recordings whose network outputs are resident.
//
// Replaces
//   gen_submission_list_task2_OLD  utility_functions.py:158-181   (threshold + decode, rows [frame, class, x, y, z])
//   gen_submission_list_task2      utility_functions.py:184-210   (the same rows + the per-frame dict with the event index)
// as train.py:110-116 calls them on every test recording.  The reference walks frames and slots in Python; here it is an
// order-preserving stream compaction in two phases, because the number of rows depends on the data:
//   count  one wave per CHUNK of 64 consecutive frames of the flattened (recording, frame) axis; lanes = slots; a frame's
//          activity is a 64-bit ballot, kept by the lane whose index is the frame's position in the chunk.  The wave
//          stores the 64 masks (8 bytes per frame, so that `sed` is read exactly once in all) and the chunk's row count.
//   scan   one workgroup turns the chunk counts into exclusive int64 row offsets and leaves the total in workspace[0].
//          It walks the counts in dependent tiles of 1024: 5 tiles at 500 x 600 frames, but 32768 serial tiles at the
//          2^31 - 1 frames the entries accept; sized for test sets, not for that limit.
//   write  one wave per chunk: lane = frame for the exclusive prefix of the 64 popcounts (-> rec_offsets where a
//          recording starts), then lane = ROW: row i of the chunk finds its frame by a 6-step search of the prefixes
//          and its slot as the (i - prefix)-th set bit of that frame's mask, fetches the slot's three coordinates (the
//          only read of `doa`, active slots only), and the 64 rows of a pass leave through LDS as 320 consecutive doubles
//          (five fully coalesced 512-byte stores instead of 64 strided 40-byte ones).
// No atomics anywhere: every output element has one writer and one value, so results repeat bit for bit.
//
// Semantics kept on purpose (the rule of metrics.hip and oracle.decode_events):
//   * a slot is active when rint(sed) != 0 (half to even: 0.5 off, 1.5 on, -0.6 on) and the frame's rounded activities
//     do not sum to zero (a frame holding -1 and +1 is dropped).  The sum only matters when a rounded value is
//     negative; it is then taken in the input's precision, which is exact in any order while every partial sum stays
//     below 2^24, i.e. for |sed| < 2^18 at the 64 slots supported here.  Nothing is promised beyond that.
//   * float32 input: x = double(float(doa) * float(max_loc_value)), one float32 multiply then widened, as numpy's
//     `l * max_loc_value`; float64 input multiplies in double.
//   * slot j is class j / overlaps, event j % overlaps.
#include "common.h"

namespace seld {

constexpr int DEC_CHUNK = 64;           // frames per wave = lanes
constexpr int DEC_WAVES = 4;            // waves per workgroup
constexpr int DEC_INFLIGHT = 16;        // rows of sed a wave has in flight (a chunk is one wave: the loads hide the latency)
constexpr int DEC_SCAN_THREADS = 1024;

// workspace: [0] total rows | [1] reserved | chunk_off[chunks] (int64) | masks[frames] (u64) | chunk_cnt[chunks] (int32)
struct DecodeWs {
    long long* total;
    long long* chunk_off;
    unsigned long long* masks;
    int* chunk_cnt;
};

__host__ __device__ inline long long decode_chunks(long long frames) { return (frames + DEC_CHUNK - 1) / DEC_CHUNK; }

inline size_t decode_ws_bytes(long long frames) {
    const long long c = decode_chunks(frames);
    return (size_t)(16 + 8 * c + 8 * frames + 4 * ((c + 1) & ~1ll));
}

inline DecodeWs decode_ws(void* ws, long long frames) {
    const long long c = decode_chunks(frames);
    DecodeWs w;
    w.total = reinterpret_cast<long long*>(ws);
    w.chunk_off = w.total + 2;
    w.masks = reinterpret_cast<unsigned long long*>(w.chunk_off + c);
    w.chunk_cnt = reinterpret_cast<int*>(w.masks + frames);
    return w;
}

// The lanes of one wave exchange data through LDS: the wave's LDS operations execute in order, so all that is needed is
// that the compiler keeps the stores before and the loads after this point.
__device__ __forceinline__ void dec_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T> __device__ __forceinline__ T dec_rint(T v);
template <> __device__ __forceinline__ float dec_rint<float>(float v) { return rintf(v); }
template <> __device__ __forceinline__ double dec_rint<double>(double v) { return rint(v); }

template <typename T> __device__ __forceinline__ T dec_wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- count: masks + rows per chunk -----------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64 * DEC_WAVES) void decode_count_kernel(const T* __restrict__ sed, long long frames, int n,
                                                                     unsigned long long* __restrict__ masks,
                                                                     int* __restrict__ chunk_cnt) {
    const int lane = threadIdx.x & 63;
    const long long chunk = (long long)blockIdx.x * DEC_WAVES + (threadIdx.x >> 6);
    const long long g0 = chunk * DEC_CHUNK;
    if (g0 >= frames) return;                                   // wave-uniform
    const int nf = (int)min((long long)DEC_CHUNK, frames - g0);
    const T* row = sed + (size_t)g0 * n;
    unsigned long long mine = 0ull;                             // the mask of frame g0 + lane
    for (int fb = 0; fb < nf; fb += DEC_INFLIGHT) {
        T v[DEC_INFLIGHT];
#pragma unroll
        for (int k = 0; k < DEC_INFLIGHT; ++k) {                // rows in flight, addresses clamped to the chunk
            const int f = min(fb + k, nf - 1);
            v[k] = lane < n ? row[(size_t)f * n + lane] : (T)0;
        }
#pragma unroll
        for (int k = 0; k < DEC_INFLIGHT; ++k) {
            if (fb + k >= nf) break;                            // uniform
            const T r = dec_rint<T>(v[k]);                      // half to even, as np.round
            unsigned long long b = __ballot(r != (T)0);
            // all rounded values >= 0: their sum is zero only when the mask is empty already
            if (__ballot(r < (T)0) != 0ull && dec_wave_sum<T>(r) == (T)0) b = 0ull;
            if (lane == fb + k) mine = b;
        }
    }
    if (lane < nf) masks[g0 + lane] = mine;
    int c = __popcll(mine);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) chunk_cnt[chunk] = c;
}

// ---- scan: exclusive int64 offsets of the chunks, total in total[0] ---------------------------------------------------
__global__ __launch_bounds__(DEC_SCAN_THREADS) void decode_scan_kernel(const int* __restrict__ chunk_cnt, long long chunks,
                                                                       long long* __restrict__ chunk_off,
                                                                       long long* __restrict__ total) {
    __shared__ long long wave_tot[DEC_SCAN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long carry = 0;
    for (long long base = 0; base < chunks; base += DEC_SCAN_THREADS) {
        const long long i = base + tid;
        const long long mine = i < chunks ? (long long)chunk_cnt[i] : 0ll;
        long long incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        long long before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < DEC_SCAN_THREADS / 64; ++w) {
            const long long t = wave_tot[w];
            before += w < wave ? t : 0ll;
            all += t;
        }
        if (i < chunks) chunk_off[i] = carry + before + incl - mine;
        carry += all;
        __syncthreads();                                        // wave_tot is rewritten by the next tile
    }
    if (tid == 0) total[0] = carry;
}

// ---- write: rows, event index, recording offsets ------------------------------------------------------------------------
template <typename T> struct __attribute__((packed, aligned(sizeof(T)))) DecXyz {
    T v[3];                                                     // one 12-byte (24-byte) load, element aligned
};

template <typename T> __device__ __forceinline__ double dec_scale(T v, double max_loc);
template <> __device__ __forceinline__ double dec_scale<float>(float v, double max_loc) { return (double)(v * (float)max_loc); }
template <> __device__ __forceinline__ double dec_scale<double>(double v, double max_loc) { return v * max_loc; }

template <typename T>
__global__ __launch_bounds__(64 * DEC_WAVES) void decode_write_kernel(const T* __restrict__ doa, long long recordings,
                                                                     int frames_per_rec, int n, int overlaps, double max_loc,
                                                                     const unsigned long long* __restrict__ masks,
                                                                     const long long* __restrict__ chunk_off,
                                                                     const long long* __restrict__ total,
                                                                     double* __restrict__ rows, int* __restrict__ event,
                                                                     long long capacity, long long* __restrict__ rec_offsets) {
    __shared__ unsigned long long mask_s[DEC_WAVES][DEC_CHUNK];
    __shared__ int excl_s[DEC_WAVES][DEC_CHUNK];
    __shared__ double stage_s[DEC_WAVES][DEC_CHUNK * 5];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long frames = recordings * frames_per_rec;
    const long long chunk = (long long)blockIdx.x * DEC_WAVES + wave;
    const long long g0 = chunk * DEC_CHUNK;
    if (g0 >= frames) return;                                   // wave-uniform; no workgroup barrier below
    const long long g = g0 + lane;
    const unsigned long long m = g < frames ? masks[g] : 0ull;
    const int cnt = __popcll(m);
    int incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
    }
    const int tot = __shfl(incl, 63, 64);
    const long long base = chunk_off[chunk];
    if (g < frames && g % frames_per_rec == 0) rec_offsets[g / frames_per_rec] = base + (incl - cnt);
    if (g == frames - 1) rec_offsets[recordings] = total[0];
    mask_s[wave][lane] = m;
    excl_s[wave][lane] = incl - cnt;
    dec_wave_sync();

    for (int i0 = 0; i0 < tot; i0 += 64) {
        const int i = i0 + lane;
        const bool valid = i < tot && base + i < capacity;
        if (valid) {
            int k = 0;                                          // the last frame whose prefix is <= i: it owns row i
#pragma unroll
            for (int s = 32; s > 0; s >>= 1)
                if (excl_s[wave][k + s] <= i) k += s;
            const unsigned long long fm = mask_s[wave][k];
            int r = i - excl_s[wave][k], j = 0;                 // slot = position of the r-th set bit of the frame's mask
#pragma unroll
            for (int w = 32; w > 0; w >>= 1) {
                const int c = __popcll((fm >> j) & ((1ull << w) - 1ull));
                if (r >= c) {
                    r -= c;
                    j += w;
                }
            }
            const long long gf = g0 + k;
            const DecXyz<T> q = *reinterpret_cast<const DecXyz<T>*>(doa + ((size_t)gf * n + j) * 3);
            double* st = &stage_s[wave][lane * 5];
            st[0] = (double)(int)(gf % frames_per_rec);
            st[1] = (double)(j / overlaps);
            st[2] = dec_scale<T>(q.v[0], max_loc);
            st[3] = dec_scale<T>(q.v[1], max_loc);
            st[4] = dec_scale<T>(q.v[2], max_loc);
            event[base + i] = j % overlaps;
        }
        dec_wave_sync();
        const long long pass_rows = min((long long)min(64, tot - i0), capacity - (base + i0));
        double* dst = rows + (size_t)(base + i0) * 5;
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const int e = q * 64 + lane;
            if (e < pass_rows * 5) dst[e] = stage_s[wave][e];
        }
        dec_wave_sync();                                        // the stage is rewritten by the next pass
    }
}

static int decode_check(int64_t recordings, int32_t frames, int32_t classes, int32_t overlaps, int32_t dtype) {
    if (recordings <= 0 || frames <= 0 || classes <= 0 || overlaps <= 0) return SELD_EINVAL;
    if (dtype != SELD_DECODE_F32 && dtype != SELD_DECODE_F64) return SELD_EINVAL;
    if ((int64_t)classes * overlaps > 64) return SELD_EUNSUPPORTED;              // one wave's ballot
    if (recordings > (int64_t)0x7fffffff / frames) return SELD_EUNSUPPORTED;       // flattened frame index fits 31 bits
    return SELD_OK;
}

}  // namespace seld

using namespace seld;

extern "C" size_t seld_decode_workspace(int64_t recordings, int32_t frames, int32_t classes, int32_t overlaps) {
    if (decode_check(recordings, frames, classes, overlaps, SELD_DECODE_F32) != SELD_OK) return 0;
    return decode_ws_bytes(recordings * frames);
}

extern "C" int seld_decode_count(const void* sed, int32_t dtype, int64_t recordings, int32_t frames, int32_t classes,
                                 int32_t overlaps, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = decode_check(recordings, frames, classes, overlaps, dtype);
    if (rc != SELD_OK) return rc;
    if (!sed) return SELD_EINVAL;
    const long long total_frames = recordings * frames;
    if (!workspace || workspace_bytes < decode_ws_bytes(total_frames)) return SELD_EWORKSPACE;
    const DecodeWs w = decode_ws(workspace, total_frames);
    const long long chunks = decode_chunks(total_frames);
    const dim3 grid((unsigned)((chunks + DEC_WAVES - 1) / DEC_WAVES)), block(64 * DEC_WAVES);
    const int n = classes * overlaps;
    if (dtype == SELD_DECODE_F32)
        hipLaunchKernelGGL(decode_count_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)sed, total_frames, n,
                           w.masks, w.chunk_cnt);
    else
        hipLaunchKernelGGL(decode_count_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)sed, total_frames, n,
                           w.masks, w.chunk_cnt);
    int lrc = check_launch();
    if (lrc != SELD_OK) return lrc;
    hipLaunchKernelGGL(decode_scan_kernel, dim3(1), dim3(DEC_SCAN_THREADS), 0, (hipStream_t)stream, w.chunk_cnt, chunks,
                       w.chunk_off, w.total);
    return check_launch();
}

extern "C" int seld_decode_write(const void* doa, int32_t dtype, int64_t recordings, int32_t frames, int32_t classes,
                                 int32_t overlaps, double max_loc_value, const void* workspace, size_t workspace_bytes,
                                 double* rows, int32_t* event, int64_t capacity, int64_t* rec_offsets, void* stream) {
    const int rc = decode_check(recordings, frames, classes, overlaps, dtype);
    if (rc != SELD_OK) return rc;
    if (capacity < 0 || !doa || !rec_offsets || (capacity > 0 && (!rows || !event))) return SELD_EINVAL;
    const long long total_frames = recordings * frames;
    if (!workspace || workspace_bytes < decode_ws_bytes(total_frames)) return SELD_EWORKSPACE;
    const DecodeWs w = decode_ws(const_cast<void*>(workspace), total_frames);
    const long long chunks = decode_chunks(total_frames);
    const dim3 grid((unsigned)((chunks + DEC_WAVES - 1) / DEC_WAVES)), block(64 * DEC_WAVES);
    const int n = classes * overlaps;
    if (dtype == SELD_DECODE_F32)
        hipLaunchKernelGGL(decode_write_kernel<float>, grid, block, 0, (hipStream_t)stream, (const float*)doa, (long long)recordings,
                           frames, n, overlaps, max_loc_value, w.masks, w.chunk_off, w.total, rows, event, (long long)capacity,
                           reinterpret_cast<long long*>(rec_offsets));
    else
        hipLaunchKernelGGL(decode_write_kernel<double>, grid, block, 0, (hipStream_t)stream, (const double*)doa, (long long)recordings,
                           frames, n, overlaps, max_loc_value, w.masks, w.chunk_off, w.total, rows, event, (long long)capacity,
                           reinterpret_cast<long long*>(rec_offsets));
    return check_launch();
}
