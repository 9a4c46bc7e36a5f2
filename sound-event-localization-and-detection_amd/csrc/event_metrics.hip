// Scoring event lists on the device: the public surface of the reference's metrics.py (task 2) and
// Dcase21_metrics.py for rows [frame, class, x, y, z] as decode.hip writes them.
//
// Replaces, for a batch of recordings given as two row lists with CSR offsets (prediction and reference):
//   location_sensitive_detection   metrics.py:123-208             (frame-wise TP / FP / FN with a distance threshold)
//   sed_score_computation          metrics.py:211-288             (the same matching on the class alone)
//   segment_labels                 Dcase21_metrics.py:239-278     (blocks of `frames_per_block` frames, class-wise)
//   SELDMetrics.update_seld_scores Dcase21_metrics.py:51-154      (track association, DCASE21 counters)
// metrics.hip does this from dense network outputs and decodes them itself; here the lists are the input, so rows from a
// CSV file, from a post-processing step or from another model can be scored.  The DCASE21 arithmetic is the code of
// metrics_common.h in both files.
//
// Rows of one recording are sorted by frame (the caller's duty; decode.hip's output is).  The order of the rows inside a
// frame is kept as given: the position of an event in its frame's list of its class is its track.
//
// Two kernels per call:
//   event_check_kernel    one thread per row: rows whose frame is no integer in [0, n_frames) -> flags[0]; the fourth
//                         event of a (recording, frame, class) cell the DCASE part would read -> flags[1].
//   event_metrics_kernel  starts only when flags[1] is zero (a refused call adds nothing).  One wave owns one (recording,
//                         block) unit at a time: it finds the unit's rows by bisection of the sorted frame column, copies
//                         them to LDS with coalesced 8-byte loads (40-byte rows: nothing wider is aligned), and works on
//                         the copy.  A unit with more than EV_CAP rows on one side is read from memory in place by the
//                         same code.  Counters stay in registers; 16 + 1 atomics per wave at the end.
#include "metrics_common.h"

namespace seld {

constexpr int EV_COUNTERS = 16;     // the 13 of metrics.hip | TP FP FN of sed_score_computation
constexpr int EV_CAP = 256;         // rows of one side of a unit staged in LDS (2 x 10 KB per wave)

struct EventP {
    const double* pred;             // (pred_n, 5)
    const long long* pred_off;      // (recordings + 1)
    long long pred_n;
    const double* tru;
    const long long* true_off;
    long long true_n;
    long long recordings, blocks;
    int n_frames, classes, fpb;
    double spatial_threshold, doa_threshold;
    long long* counters;
    double* total_de;
    long long* flags;
};

// rows off[r] .. off[r + 1] of recording r, forced into [0, n] and into ascending order: whatever the offsets hold, no
// row outside the list is read
__device__ __forceinline__ void rec_range(const long long* off, long long r, long long n, long long& lo, long long& hi) {
    lo = min(max(off[r], 0ll), n);
    hi = min(max(off[r + 1], lo), n);
}

// first row in [lo, hi) whose frame is not below `key` (a NaN frame counts as not below)
template <class Index>
__device__ __forceinline__ Index first_frame_not_below(const double* rows, Index lo, Index hi, double key) {
    while (lo < hi) {
        const Index mid = lo + (hi - lo) / 2;
        if (rows[mid * 5] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool whole_in(double f, double lo, double hi) { return f >= lo && f < hi && f == floor(f); }

__global__ __launch_bounds__(256) void event_check_kernel(const EventP p) {
    const long long total = p.pred_n + p.true_n;
    const double dcase_end = (double)p.blocks * (double)p.fpb;
    long long bad_frame = 0, bad_cell = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const bool is_pred = i < p.pred_n;
        const double* rows = is_pred ? p.pred : p.tru;
        const long long* off = is_pred ? p.pred_off : p.true_off;
        const long long n = is_pred ? p.pred_n : p.true_n;
        const long long row = is_pred ? i : i - p.pred_n;
        // the recording of the row: the last r with off[r] <= row
        long long a = 0, b = p.recordings + 1;
        while (a < b) {
            const long long mid = a + (b - a) / 2;
            if (off[mid] <= row) a = mid + 1; else b = mid;
        }
        if (a == 0 || a > p.recordings) continue;       // before the first or behind the last recording: nobody's row
        long long lo, hi;
        rec_range(off, a - 1, n, lo, hi);
        if (row < lo || row >= hi) continue;
        const double f = rows[row * 5], c = rows[row * 5 + 1];
        if (!whole_in(f, 0.0, (double)p.n_frames)) ++bad_frame;
        if (whole_in(f, 0.0, dcase_end) && whole_in(c, 0.0, (double)p.classes)) {
            int earlier = 0;                            // events of the same cell in front of this one
            for (long long j = row - 1; j >= lo && rows[j * 5] == f && earlier <= 3; --j) earlier += rows[j * 5 + 1] == c ? 1 : 0;
            if (earlier == 3) ++bad_cell;               // the fourth event of its cell: every overflowing cell has one
        }
    }
    bad_frame = wave_sum_i64(bad_frame);
    bad_cell = wave_sum_i64(bad_cell);
    if ((threadIdx.x & 63) == 0) {
        if (bad_frame) atomicAdd(reinterpret_cast<unsigned long long*>(p.flags), (unsigned long long)bad_frame);
        if (bad_cell) atomicAdd(reinterpret_cast<unsigned long long*>(p.flags + 1), (unsigned long long)bad_cell);
    }
}

// One unit: P (np rows) and T (nt rows) are the predictions and references of one recording whose frames lie in the
// block [f0, f0 + fpb), each sorted by frame; in LDS or in memory (inlined once for each).
__device__ __forceinline__ void score_unit(const double* P, int np, const double* T, int nt, const EventP& p, double f0, int lane,
                                           long long (&cnt)[EV_COUNTERS], double& total_de) {
    // ---- location_sensitive_detection and sed_score_computation: lane = row ----
    // Per frame: no reference -> FP += 2 p; no prediction -> FN += 2 t; else TP += m, FN += t - m, FP += p - m.  Row by
    // row that is: a prediction adds 1 to FP (2 where its frame has no reference), a reference adds 2 to FN where its
    // frame has no prediction, else TP + 1 and FP - 1 when matched, FN + 1 when not.  cnt[13..15] the same on the class alone.
    const double lsd_end = (double)p.n_frames;
    for (int i = lane; i < np; i += 64) {
        const double f = P[i * 5];
        if (!whole_in(f, 0.0, lsd_end)) continue;
        const int j = first_frame_not_below(T, 0, nt, f);
        const int add = (j < nt && T[j * 5] == f) ? 1 : 2;
        cnt[1] += add;
        cnt[14] += add;
    }
    for (int i = lane; i < nt; i += 64) {
        const double f = T[i * 5];
        if (!whole_in(f, 0.0, lsd_end)) continue;
        int j = first_frame_not_below(P, 0, np, f);
        if (!(j < np && P[j * 5] == f)) {
            cnt[2] += 2;
            cnt[15] += 2;
            continue;
        }
        const double c = T[i * 5 + 1], x = T[i * 5 + 2], y = T[i * 5 + 3], z = T[i * 5 + 4];
        bool near = false, same = false;
        for (; j < np && P[j * 5] == f; ++j) {
            if (P[j * 5 + 1] != c) continue;
            same = true;
            const double dx = x - P[j * 5 + 2], dy = y - P[j * 5 + 3], dz = z - P[j * 5 + 4];
            if (sqrt(dx * dx + dy * dy + dz * dz) < p.spatial_threshold) near = true;
        }
        cnt[0] += near ? 1 : 0;
        cnt[1] -= near ? 1 : 0;
        cnt[2] += near ? 0 : 1;
        cnt[13] += same ? 1 : 0;
        cnt[14] -= same ? 1 : 0;
        cnt[15] += same ? 0 : 1;
    }
    if (p.classes == 0) return;

    // ---- DCASE21 block metrics: lane = class ----
    // Every lane walks the two lists together, frame by frame in ascending order, and keeps the events of its own class:
    // up to 3 references g and 3 predictions q of the frame in registers, the longest list of each side, and per
    // reference track the sum and count of its matched distances.
    const double mine = lane < p.classes ? (double)lane : __builtin_nan("");      // NaN equals no class
    int ip = 0, it = 0, nb_gt = 0, nb_pred = 0, n0 = 0, n1 = 0, n2 = 0;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    while (ip < np || it < nt) {
        const double fp = ip < np ? P[ip * 5] : __builtin_inf(), ft = it < nt ? T[it * 5] : __builtin_inf();
        if (fp != fp) { ++ip; continue; }               // a NaN frame belongs to no block: stepped over, wherever it sorts
        if (ft != ft) { ++it; continue; }
        const double f = fmin(fp, ft);
        const bool frame_ok = whole_in(f, f0, f0 + (double)p.fpb);
        double ga[3][3], qa[3][3];
        int g = 0, q = 0;
        for (; it < nt && !(T[it * 5] > f); ++it) {      // not above: a NaN frame is stepped over, never waited for
            if (!(frame_ok && T[it * 5] == f && T[it * 5 + 1] == mine)) continue;
#pragma unroll
            for (int e = 0; e < 3; ++e)
                if (g == e) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) ga[e][k] = T[it * 5 + 2 + k];
                }
            ++g;
        }
        for (; ip < np && !(P[ip * 5] > f); ++ip) {
            if (!(frame_ok && P[ip * 5] == f && P[ip * 5 + 1] == mine)) continue;
#pragma unroll
            for (int e = 0; e < 3; ++e)
                if (q == e) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) qa[e][k] = P[ip * 5 + 2 + k];
                }
            ++q;
        }
        g = min(g, 3);                                  // a longer list is refused by event_check_kernel before this runs
        q = min(q, 3);
        nb_gt = max(nb_gt, g);
        nb_pred = max(nb_pred, q);
        if (g && q) {
            double cost[9];
#pragma unroll
            for (int e = 0; e < 3; ++e)
#pragma unroll
                for (int e2 = 0; e2 < 3; ++e2) cost[e * 3 + e2] = (e < g && e2 < q) ? angular_distance_deg(ga[e], qa[e2]) : 0.0;
            double o0 = -1.0, o1 = -1.0, o2 = -1.0;
            assign_3x3((1u << g) - 1u, (1u << q) - 1u, cost, o0, o1, o2);
            if (o0 >= 0.0) { s0 += o0; ++n0; }
            if (o1 >= 0.0) { s1 += o1; ++n1; }
            if (o2 >= 0.0) { s2 += o2; ++n2; }
        }
    }
    int loc_fn = 0, loc_fp = 0;
    if (lane < p.classes) {
        const DcaseAdd a = dcase_class_block(nb_gt, nb_pred, s0, s1, s2, n0, n1, n2, p.doa_threshold, total_de);
        SELD_DCASE_ADD(cnt, a);
        loc_fn = a.fn;
        loc_fp = a.fp;
    }
    const int blk_fn = wave_sum_i32(loc_fn), blk_fp = wave_sum_i32(loc_fp);
    if (lane == 0) {
        cnt[6] += min(blk_fp, blk_fn);
        cnt[7] += max(0, blk_fn - blk_fp);
        cnt[8] += max(0, blk_fp - blk_fn);
    }
}

__global__ __launch_bounds__(64) void event_metrics_kernel(const EventP p) {
    __shared__ __attribute__((aligned(16))) double pred_s[EV_CAP * 5];
    __shared__ __attribute__((aligned(16))) double true_s[EV_CAP * 5];
    if (p.flags[1] != 0) return;                        // refused by event_check_kernel: nothing is added
    const int lane = threadIdx.x;
    long long cnt[EV_COUNTERS];
#pragma unroll
    for (int i = 0; i < EV_COUNTERS; ++i) cnt[i] = 0;   // lane-local partial sums, reduced over the wave at the end
    double total_de = 0.0;
    const long long total = p.recordings * p.blocks;
    for (long long u = blockIdx.x; u < total; u += gridDim.x) {
        const long long rec = u / p.blocks, blk = u % p.blocks;
        const double f0 = (double)blk * (double)p.fpb, f1 = f0 + (double)p.fpb;
        long long plo = 0, phi = 0, tlo = 0, thi = 0;
        if (p.pred_n) rec_range(p.pred_off, rec, p.pred_n, plo, phi);
        if (p.true_n) rec_range(p.true_off, rec, p.true_n, tlo, thi);
        const long long p0 = first_frame_not_below(p.pred, plo, phi, f0), p1 = first_frame_not_below(p.pred, p0, phi, f1);
        const long long t0 = first_frame_not_below(p.tru, tlo, thi, f0), t1 = first_frame_not_below(p.tru, t0, thi, f1);
        const int np = (int)(p1 - p0), nt = (int)(t1 - t0);
        if (np == 0 && nt == 0) continue;
        if (np <= EV_CAP && nt <= EV_CAP) {
            for (int i = lane; i < np * 5; i += 64) pred_s[i] = p.pred[p0 * 5 + i];
            for (int i = lane; i < nt * 5; i += 64) true_s[i] = p.tru[t0 * 5 + i];
            __syncthreads();
            score_unit(pred_s, np, true_s, nt, p, f0, lane, cnt, total_de);
            __syncthreads();                            // the copy is rewritten by the next unit
        } else {
            score_unit(p.pred + p0 * 5, np, p.tru + t0 * 5, nt, p, f0, lane, cnt, total_de);
        }
    }
#pragma unroll
    for (int i = 0; i < EV_COUNTERS; ++i) {
        const long long s = wave_sum_i64(cnt[i]);
        if (lane == 0 && s != 0) atomicAdd(reinterpret_cast<unsigned long long*>(p.counters + i), (unsigned long long)s);
    }
    const double de = wave_sum_d(total_de);
    if (lane == 0 && de != 0.0) atomicAdd(p.total_de, de);
}

}  // namespace seld

using namespace seld;

extern "C" int seld_event_metrics_accumulate(const double* pred_rows, const int64_t* pred_offsets, int64_t pred_count,
                                             const double* true_rows, const int64_t* true_offsets, int64_t true_count,
                                             int64_t recordings, int32_t n_frames, int32_t nb_classes, int32_t frames_per_block,
                                             double spatial_threshold, double doa_threshold, int64_t* counters,
                                             double* total_de, int64_t* flags, void* stream) {
    if (recordings < 0 || pred_count < 0 || true_count < 0 || n_frames < 0 || !counters || !total_de || !flags) return SELD_EINVAL;
    if (nb_classes < 0 || nb_classes > 64 || frames_per_block < 1) return SELD_EINVAL;
    if (pred_count > 0x0fffffff || true_count > 0x0fffffff) return SELD_EUNSUPPORTED;    // 5 * row index stays an int inside a unit
    if ((pred_count && (!pred_rows || !pred_offsets)) || (true_count && (!true_rows || !true_offsets))) return SELD_EINVAL;
    const hipError_t e = hipMemsetAsync(flags, 0, 2 * sizeof(int64_t), (hipStream_t)stream);
    if (e != hipSuccess) {
        g_last_hip_error = (int)e;
        return SELD_ELAUNCH;
    }
    if (recordings == 0) return SELD_OK;
    EventP p;
    p.pred = pred_rows;
    p.pred_off = reinterpret_cast<const long long*>(pred_offsets);
    p.pred_n = pred_count;
    p.tru = true_rows;
    p.true_off = reinterpret_cast<const long long*>(true_offsets);
    p.true_n = true_count;
    p.recordings = recordings;
    p.blocks = ((long long)n_frames + frames_per_block - 1) / frames_per_block;
    p.n_frames = n_frames;
    p.classes = nb_classes;
    p.fpb = frames_per_block;
    p.spatial_threshold = spatial_threshold;
    p.doa_threshold = doa_threshold;
    p.counters = reinterpret_cast<long long*>(counters);
    p.total_de = total_de;
    p.flags = reinterpret_cast<long long*>(flags);
    const long long rows = pred_count + true_count;
    if (rows == 0) return SELD_OK;                      // nothing to check, and every unit is empty
    long long wgs = (rows + 255) / 256;
    if (wgs > 2048) wgs = 2048;
    hipLaunchKernelGGL(event_check_kernel, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream, p);
    const int rc = check_launch();
    if (rc != SELD_OK) return rc;
    const long long total = recordings * p.blocks;
    if (total == 0) return SELD_OK;
    wgs = total > 4096 ? 4096 : total;                  // 2 generations of resident waves; waves loop over their units
    hipLaunchKernelGGL(event_metrics_kernel, dim3((unsigned)wgs), dim3(64), 0, (hipStream_t)stream, p);
    return check_launch();
}
