// Track post-processing on the device: median filter, hysteresis, gap fill, minimum duration and one DOA per event
// (seld_smooth_tracks), and the event list of any track (seld_track_events_*).  include/seld_hip.h has the definitions.
//
// seld_smooth_tracks: ONE launch, one 256-thread workgroup per column (r, j), the column's T frames resident in LDS from
// the first read to the last write.  The rules are sequential along time when written naively; here every one of them is a
// pair of scans over frames:
//   median     thread = frame (t = tid, tid + 256, ...): the window's median by rank counting over the staged column --
//              candidate v is the median when  #{w < v} <= h < #{w <= v} ; median^2 compares, exact, no sort.
//   run rules  thread = CHUNK of `len` consecutive frames (len odd: the chunk stride then spreads over the LDS banks).  A
//              forward pass gives every frame the start `lo` of its maximal run (an inclusive max-scan of the positions
//              where the flag changes), a backward pass its exclusive end `hi` (a min-scan from the right).  Either pass is
//              a walk over the thread's chunk for the chunk's summary, one 256-entry workgroup scan of the summaries (wave
//              shuffles + four wave totals through LDS), and a second walk that carries the scanned value and consumes it
//              on the spot.
//                hysteresis   also scans "last frame above `on` at or before t" / "first one at or after t": the run
//                             [lo, hi) of p > off is kept iff one of them falls inside it
//                gap fill     an inactive run with 0 < lo, hi < T and hi - lo <= max_gap becomes active
//                duration     an active run with hi - lo < min_frames becomes inactive; lo and hi of the surviving runs
//                             stay in LDS for the DOAs
//   DOAs       every thread sums  w * d  (double) over the pieces of runs inside its chunk, in frame order.  A run inside
//              one chunk is finished and written by its thread.  Of a run that crosses chunks, the thread that holds its
//              first frame keeps its own piece in registers, every later chunk leaves its piece (the one touching the
//              chunk's start) in LDS, and the first thread adds those in chunk order, divides once and leaves the three
//              floats in LDS for the threads of the other chunks.  A fixed order, no term from outside the run, no atomics.
// LDS: 9 T bytes (p, two uint16 position arrays that first hold the raw column, one activity byte) + 12.3 KB; T = 16384
// takes 159.9 KB of the CU's 160, the common 600 frames 17.7 KB.  The column's global reads and writes are strided by n
// floats: neighbouring columns re-touch each 64-byte sector, which the caches are left to absorb (DESIGN.md has the rate).
//
// seld_track_events_*: the two-call pattern of decode.hip.  One thread per (recording, segment of 64 frames, column), the
// column fastest so that a wave reads whole rows of `sed`; a thread owns the runs that START in its segment.  count: runs
// per (recording, column, segment) in row order; decode.hip's scan kernel turns them into int64 offsets and the total;
// write: the thread walks each of its runs to its end (beyond the segment if need be), sums the DOAs in double and
// writes the row.  No atomics.
#include <cmath>

#include "common.h"

namespace seld {

// csrc/decode.hip: exclusive int64 offsets of `chunks` int32 counts by one workgroup of 1024, the total in total[0]
__global__ void decode_scan_kernel(const int* __restrict__ chunk_cnt, long long chunks, long long* __restrict__ chunk_off,
                                   long long* __restrict__ total);

constexpr int SM_THREADS = 256;
constexpr int SM_WAVES = SM_THREADS / 64;
constexpr int SM_INF = 0x7fffffff;
constexpr size_t SM_LDS_DEFAULT = 64 * 1024;         // above this the launch needs hipFuncAttributeMaxDynamicSharedMemorySize

struct SmSums {
    double w, x, y, z;
};

struct __attribute__((packed, aligned(4))) SmXyz {
    float v[3];                                                 // a column's DOA of one frame: one 12-byte load or store
};
__device__ __forceinline__ SmXyz sm_load3(const float* p) { return *reinterpret_cast<const SmXyz*>(p); }
__device__ __forceinline__ void sm_store3(float* p, const SmXyz& q) { *reinterpret_cast<SmXyz*>(p) = q; }

// bytes: p[T] float | A[T] u16 | B[T] u16 (A and B first hold the raw column as T floats) | act[T] u8, padded to 16 |
//        lead[256] SmSums | res[256] float4 | scan[SM_WAVES] int
__host__ __device__ inline size_t sm_lds_var(int T) { return ((size_t)9 * T + 15) & ~(size_t)15; }
inline size_t sm_lds_bytes(int T) { return sm_lds_var(T) + SM_THREADS * (sizeof(SmSums) + sizeof(float4)) + 64; }

// max over the threads before this one (forward) / min over the threads after it (backward); `scan` is rewritten per call
__device__ __forceinline__ int sm_excl_max_fwd(int v, int* scan) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(incl, o, 64);
        if (lane >= o) incl = max(incl, u);
    }
    int excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0;
    __syncthreads();                                            // the previous call's readers are done with `scan`
    if (lane == 63) scan[wave] = incl;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < SM_WAVES; ++w)
        if (w < wave) excl = max(excl, scan[w]);
    return excl;
}

__device__ __forceinline__ int sm_excl_min_bwd(int v, int* scan) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_down(incl, o, 64);
        if (lane + o < 64) incl = min(incl, u);
    }
    int excl = __shfl_down(incl, 1, 64);
    if (lane == 63) excl = SM_INF;
    __syncthreads();
    if (lane == 0) scan[wave] = incl;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < SM_WAVES; ++w)
        if (w > wave) excl = min(excl, scan[w]);
    return excl;
}

// One pair of passes over a 0/1 flag f(t): fwd(t, lo) for every frame of the chunk in ascending order, then bwd(t, hi) in
// descending order; [lo, hi) is the maximal run of equal flags that holds t.  What fwd and bwd write must not be what f
// reads: other threads evaluate f at this chunk's edge frames meanwhile.
template <typename Flag, typename Fwd, typename Bwd>
__device__ __forceinline__ void sm_runs(int T, int b, int e, int* scan, Flag f, Fwd fwd, Bwd bwd) {
    int best = 0;                                               // frame 0 starts a run: position 0 is the identity
    for (int t = b; t < e; ++t)
        if (t > 0 && f(t) != f(t - 1)) best = t;
    int lo = sm_excl_max_fwd(best, scan);
    for (int t = b; t < e; ++t) {
        if (t > 0 && f(t) != f(t - 1)) lo = t;
        fwd(t, lo);
    }
    best = SM_INF;
    for (int t = e - 1; t >= b; --t)
        if (t == T - 1 || f(t + 1) != f(t)) best = min(best, t + 1);
    int hi = sm_excl_min_bwd(best, scan);
    for (int t = e - 1; t >= b; --t) {
        if (t == T - 1 || f(t + 1) != f(t)) hi = t + 1;
        bwd(t, hi);
    }
    __syncthreads();
}

__global__ __launch_bounds__(SM_THREADS) void smooth_tracks_kernel(const float* __restrict__ sed, const float* __restrict__ doa,
                                                                  int T, int n, int median, float on, float off,
                                                                  int min_frames, int max_gap, int doa_mode,
                                                                  float* __restrict__ out_sed, float* __restrict__ out_doa,
                                                                  float* __restrict__ out_prob) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_lds[];
    float* p = reinterpret_cast<float*>(sm_lds);
    float* raw = p + T;                                         // until the median is taken
    unsigned short* A = reinterpret_cast<unsigned short*>(p + T);
    unsigned short* B = A + T;
    unsigned char* act = reinterpret_cast<unsigned char*>(B + T);
    SmSums* lead = reinterpret_cast<SmSums*>(sm_lds + sm_lds_var(T));
    float4* res = reinterpret_cast<float4*>(lead + SM_THREADS);
    int* scan = reinterpret_cast<int*>(res + SM_THREADS);

    const int tid = threadIdx.x;
    // Workgroups are dealt round-robin over the 8 XCDs, each with an L2 of its own, and 16 neighbouring columns share every
    // 64-byte sector of `sed`: inside each full tile of 128 workgroups, those of one XCD take 16 consecutive columns.  A
    // bijection of the tile; only speed depends on where a workgroup really runs.
    long long col = blockIdx.x;                                 // r * n + j
    if (col < ((long long)gridDim.x & ~127ll)) {
        const int w = (int)(col & 127);
        col = (col & ~127ll) + (w & 7) * 16 + (w >> 3);
    }
    const long long r = col / n;
    const int j = (int)(col - r * n);
    const size_t sed0 = (size_t)r * T * n + j;                  // + t * n
    const size_t doa0 = (size_t)r * T * 3 * n + 3 * (size_t)j;  // + t * 3 n

    // ---- the column, then its median -------------------------------------------------------------------------------
    for (int t = tid; t < T; t += SM_THREADS) raw[t] = sed[sed0 + (size_t)t * n];
    __syncthreads();
    const int h = (median - 1) >> 1;
    for (int t = tid; t < T; t += SM_THREADS) {
        float m = raw[t];
        if (h > 0) {
            for (int a = -h; a <= h; ++a) {
                const float v = raw[min(max(t + a, 0), T - 1)];
                int less = 0, leq = 0;
                for (int c = -h; c <= h; ++c) {
                    const float w = raw[min(max(t + c, 0), T - 1)];
                    less += w < v ? 1 : 0;
                    leq += w <= v ? 1 : 0;
                }
                if (less <= h && h < leq) {
                    m = v;
                    break;
                }
            }
        }
        p[t] = m;
        if (out_prob) out_prob[sed0 + (size_t)t * n] = m;
    }
    __syncthreads();                                            // raw is dead: A and B take its place

    // ---- chunks --------------------------------------------------------------------------------------------------------
    const int len = ((T + SM_THREADS - 1) / SM_THREADS) | 1;
    const int b = min(T, tid * len), e = min(T, b + len);

    // hysteresis: runs of p > off that hold a frame with p > on.  fwd: A = "such a frame in [lo, t]"; bwd: act = a1
    {
        int last_on = 0;                                        // 1 + the last frame <= t with p > on, 0: none
        for (int t = b; t < e; ++t)
            if (p[t] > on) last_on = t + 1;
        last_on = sm_excl_max_fwd(last_on, scan);
        int next_on = SM_INF;                                   // the first frame >= t with p > on
        for (int t = e - 1; t >= b; --t)
            if (p[t] > on) next_on = t;
        next_on = sm_excl_min_bwd(next_on, scan);
        sm_runs(
            T, b, e, scan, [&](int t) { return p[t] > off; },
            [&](int t, int lo) {
                if (p[t] > on) last_on = t + 1;
                A[t] = (unsigned short)(last_on > lo ? 1 : 0);
            },
            [&](int t, int hi) {
                if (p[t] > on) next_on = t;
                act[t] = (unsigned char)((p[t] > off && (A[t] != 0 || next_on < hi)) ? 1 : 0);
            });
    }
    // gap fill: fwd: A = lo; bwd: B = a2
    sm_runs(
        T, b, e, scan, [&](int t) { return act[t] != 0; }, [&](int t, int lo) { A[t] = (unsigned short)lo; },
        [&](int t, int hi) {
            const int lo = A[t];
            const bool fill = lo > 0 && hi < T && hi - lo <= max_gap;
            B[t] = (unsigned short)((act[t] != 0 || fill) ? 1 : 0);
        });
    for (int t = b; t < e; ++t) act[t] = (unsigned char)B[t];
    __syncthreads();
    // minimum duration: fwd: A = lo; bwd: B = hi of a surviving active run, 0 on an inactive frame
    sm_runs(
        T, b, e, scan, [&](int t) { return act[t] != 0; }, [&](int t, int lo) { A[t] = (unsigned short)lo; },
        [&](int t, int hi) { B[t] = (unsigned short)((act[t] != 0 && hi - (int)A[t] >= min_frames) ? hi : 0); });

    for (int t = tid; t < T; t += SM_THREADS) out_sed[sed0 + (size_t)t * n] = B[t] != 0 ? 1.0f : 0.0f;

    // ---- DOAs --------------------------------------------------------------------------------------------------------------
    if (doa_mode == SELD_SMOOTH_DOA_FRAME) {
        for (int t = tid; t < T; t += SM_THREADS) {
            const size_t o = doa0 + (size_t)t * 3 * n;
            sm_store3(out_doa + o, sm_load3(doa + o));
        }
        return;
    }
    const bool weighted = doa_mode == SELD_SMOOTH_DOA_WEIGHTED;
    SmSums mine = {0.0, 0.0, 0.0, 0.0};                         // the piece of a run that starts in this chunk and leaves it
    int mine_hi = 0;
    for (int t = b; t < e;) {
        const size_t o = doa0 + (size_t)t * 3 * n;
        const int hi = B[t];
        if (hi == 0) {
            sm_store3(out_doa + o, sm_load3(doa + o));
            ++t;
            continue;
        }
        const int lo = A[t], pe = min(hi, e);
        SmSums s = {0.0, 0.0, 0.0, 0.0};
        for (int u = t; u < pe; ++u) {
            const SmXyz d = sm_load3(doa + doa0 + (size_t)u * 3 * n);
            const double w = weighted ? (double)p[u] : 1.0;
            s.w += w;
            s.x += w * (double)d.v[0];
            s.y += w * (double)d.v[1];
            s.z += w * (double)d.v[2];
        }
        if (lo < b) {
            lead[tid] = s;                                      // continues a run of an earlier chunk (t == b)
        } else if (hi > e) {
            mine = s;
            mine_hi = hi;
        } else {                                                // the whole run: finished here
            const SmXyz v = {{(float)(s.x / s.w), (float)(s.y / s.w), (float)(s.z / s.w)}};
            for (int u = t; u < pe; ++u) sm_store3(out_doa + doa0 + (size_t)u * 3 * n, v);
        }
        t = pe;
    }
    __syncthreads();
    if (mine_hi != 0) {
        const int last = (mine_hi - 1) / len;                   // the chunk of the run's last frame
        for (int k = tid + 1; k <= last; ++k) {
            const SmSums s = lead[k];
            mine.w += s.w;
            mine.x += s.x;
            mine.y += s.y;
            mine.z += s.z;
        }
        res[tid] = make_float4((float)(mine.x / mine.w), (float)(mine.y / mine.w), (float)(mine.z / mine.w), 0.f);
    }
    __syncthreads();
    for (int t = b; t < e; ++t) {
        const int hi = B[t];
        if (hi == 0) continue;
        const int lo = A[t];
        if (lo >= b && hi <= e) continue;                       // written above
        const float4 v = res[lo / len];
        const SmXyz q = {{v.x, v.y, v.z}};
        sm_store3(out_doa + doa0 + (size_t)t * 3 * n, q);
    }
}

// ---- event lists ---------------------------------------------------------------------------------------------------------
constexpr int TE_SEG = 64;                                      // frames of a segment
constexpr int TE_THREADS = 256;

struct TrackWs {
    long long* total;
    long long* off;
    int* cnt;
};

__host__ __device__ inline long long te_segments(int T) { return (T + TE_SEG - 1) / TE_SEG; }
inline size_t te_ws_bytes(long long items) { return (size_t)(16 + 8 * items + 4 * ((items + 1) & ~1ll)); }
inline TrackWs te_ws(void* ws, long long items) {
    TrackWs w;
    w.total = reinterpret_cast<long long*>(ws);
    w.off = w.total + 2;
    w.cnt = reinterpret_cast<int*>(w.off + items);
    return w;
}

// thread id -> (r, s, j), j fastest; the counts are indexed (r, j, s): the order of the rows
__global__ __launch_bounds__(TE_THREADS) void track_count_kernel(const float* __restrict__ sed, long long items, int T, int n,
                                                                int S, int* __restrict__ cnt) {
    const long long id = (long long)blockIdx.x * TE_THREADS + threadIdx.x;
    if (id >= items) return;
    const int j = (int)(id % n);
    const long long rs = id / n;
    const int s = (int)(rs % S);
    const long long r = rs / S;
    const float* column = sed + (size_t)r * T * n + j;
    const int t0 = s * TE_SEG, t1 = min(T, t0 + TE_SEG);
    bool before = t0 > 0 && column[(size_t)(t0 - 1) * n] > 0.5f;
    int c = 0;
    for (int t = t0; t < t1; ++t) {
        const bool a = column[(size_t)t * n] > 0.5f;
        c += (a && !before) ? 1 : 0;
        before = a;
    }
    cnt[(r * n + j) * S + s] = c;
}

__global__ __launch_bounds__(TE_THREADS) void track_write_kernel(const float* __restrict__ sed, const float* __restrict__ doa,
                                                                long long recordings, long long items, int T, int n, int S,
                                                                int overlaps, double max_loc, const long long* __restrict__ off,
                                                                const long long* __restrict__ total, double* __restrict__ rows,
                                                                long long capacity, long long* __restrict__ rec_offsets) {
    const long long id = (long long)blockIdx.x * TE_THREADS + threadIdx.x;
    if (id >= items) return;
    const int j = (int)(id % n);
    const long long rs = id / n;
    const int s = (int)(rs % S);
    const long long r = rs / S;
    long long row = off[(r * n + j) * S + s];
    if (j == 0 && s == 0) rec_offsets[r] = row;
    if (id == 0) rec_offsets[recordings] = total[0];
    const float* column = sed + (size_t)r * T * n + j;
    const float* xyz = doa + (size_t)r * T * 3 * n + 3 * (size_t)j;
    const int t0 = s * TE_SEG, t1 = min(T, t0 + TE_SEG);
    bool before = t0 > 0 && column[(size_t)(t0 - 1) * n] > 0.5f;
    for (int t = t0; t < t1; ++t) {
        const bool a = column[(size_t)t * n] > 0.5f;
        if (a && !before && row < capacity) {
            double x = 0.0, y = 0.0, z = 0.0;
            int u = t;
            do {
                const float* d = xyz + (size_t)u * 3 * n;
                x += (double)d[0];
                y += (double)d[1];
                z += (double)d[2];
                ++u;
            } while (u < T && column[(size_t)u * n] > 0.5f);
            const double len = (double)(u - t);
            double* dst = rows + (size_t)row * 8;
            dst[0] = (double)r;
            dst[1] = (double)(j / overlaps);
            dst[2] = (double)(j % overlaps);
            dst[3] = (double)t;
            dst[4] = (double)u;
            dst[5] = x / len * max_loc;
            dst[6] = y / len * max_loc;
            dst[7] = z / len * max_loc;
        }
        row += (a && !before) ? 1 : 0;
        before = a;
    }
}

static int track_check(int64_t R, int32_t T, int64_t n) {
    if (R < 1 || T < 1 || n < 1) return SELD_EINVAL;
    const long long S = te_segments(T);
    if (R > (int64_t)0x7fffffff / n || R * n > (int64_t)0x7fffffff / S) return SELD_EUNSUPPORTED;    // 31-bit thread ids
    return SELD_OK;
}

}  // namespace seld

using namespace seld;

extern "C" int seld_smooth_tracks(const float* sed, const float* doa, int64_t R, int32_t T, int32_t n, int32_t median, float on,
                                  float off, int32_t min_frames, int32_t max_gap, int32_t doa_mode, float* out_sed,
                                  float* out_doa, float* out_prob, void* stream) {
    if (!sed || !doa || !out_sed || !out_doa || R < 1 || T < 1 || n < 1) return SELD_EINVAL;
    if (median < 1 || median > SELD_SMOOTH_MAX_MEDIAN || (median & 1) == 0) return SELD_EINVAL;
    if (!std::isfinite(on) || !std::isfinite(off) || !(0.0f <= off && off <= on && on <= 1.0f)) return SELD_EINVAL;
    if (min_frames < 1 || max_gap < 0) return SELD_EINVAL;
    if (doa_mode != SELD_SMOOTH_DOA_FRAME && doa_mode != SELD_SMOOTH_DOA_MEAN && doa_mode != SELD_SMOOTH_DOA_WEIGHTED)
        return SELD_EINVAL;
    if (T > SELD_SMOOTH_MAX_FRAMES || R > (int64_t)0x7fffffff / n) return SELD_EUNSUPPORTED;
    const size_t smem = sm_lds_bytes(T);
    if (smem > SM_LDS_DEFAULT &&
        hipFuncSetAttribute((const void*)smooth_tracks_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
        return SELD_ELAUNCH;
    hipLaunchKernelGGL(smooth_tracks_kernel, dim3((unsigned)(R * n)), dim3(SM_THREADS), smem, (hipStream_t)stream, sed, doa, T, n,
                       median, on, off, min_frames, max_gap, doa_mode, out_sed, out_doa, out_prob);
    return check_launch();
}

extern "C" size_t seld_track_events_workspace(int64_t R, int32_t T, int32_t n) {
    if (track_check(R, T, n) != SELD_OK) return 0;
    return te_ws_bytes(R * n * te_segments(T));
}

extern "C" int seld_track_events_count(const float* sed, int64_t R, int32_t T, int32_t n, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    const int rc = track_check(R, T, n);
    if (rc != SELD_OK) return rc;
    if (!sed) return SELD_EINVAL;
    const long long S = te_segments(T), items = R * n * S;
    if (!workspace || workspace_bytes < te_ws_bytes(items)) return SELD_EWORKSPACE;
    const TrackWs w = te_ws(workspace, items);
    hipLaunchKernelGGL(track_count_kernel, dim3((unsigned)((items + TE_THREADS - 1) / TE_THREADS)), dim3(TE_THREADS), 0,
                       (hipStream_t)stream, sed, items, T, n, (int)S, w.cnt);
    const int lrc = check_launch();
    if (lrc != SELD_OK) return lrc;
    hipLaunchKernelGGL(decode_scan_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, w.cnt, items, w.off, w.total);
    return check_launch();
}

extern "C" int seld_track_events_write(const float* sed, const float* doa, int64_t R, int32_t T, int32_t classes,
                                       int32_t overlaps, double max_loc_value, const void* workspace, size_t workspace_bytes,
                                       double* rows, int64_t capacity, int64_t* rec_offsets, void* stream) {
    if (classes < 1 || overlaps < 1 || (int64_t)classes * overlaps > 0x7fffffff) return SELD_EINVAL;
    const int n = classes * overlaps;
    const int rc = track_check(R, T, n);
    if (rc != SELD_OK) return rc;
    if (capacity < 0 || !sed || !doa || !rec_offsets || (capacity > 0 && !rows)) return SELD_EINVAL;
    const long long S = te_segments(T), items = R * n * S;
    if (!workspace || workspace_bytes < te_ws_bytes(items)) return SELD_EWORKSPACE;
    const TrackWs w = te_ws(const_cast<void*>(workspace), items);
    hipLaunchKernelGGL(track_write_kernel, dim3((unsigned)((items + TE_THREADS - 1) / TE_THREADS)), dim3(TE_THREADS), 0,
                       (hipStream_t)stream, sed, doa, (long long)R, items, T, n, (int)S, overlaps, max_loc_value, w.off, w.total,
                       rows, (long long)capacity, reinterpret_cast<long long*>(rec_offsets));
    return check_launch();
}
