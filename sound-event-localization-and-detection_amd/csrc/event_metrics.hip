// Scoring event lists on the device: the public surface of the reference's metrics.py (task 2) and
// Dcase21_metrics.py for rows [frame, class, x, y, z] as decode.hip writes them, or [frame, class, azimuth, elevation]
// in degrees as DCASE label files give them (COORDS = 3 / 2; a row is 2 + COORDS doubles).
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
//   event_check_kernel    one thread per row: rows whose frame is no integer in [0, n_frames) -> flags[0]; event
//                         max_tracks + 1 of a (recording, frame, class) cell the DCASE part would read -> flags[1].
//   event_metrics_kernel  starts only when flags[1] is zero (a refused call adds nothing).  One wave owns one (recording,
//                         block) unit at a time: it finds the unit's rows by bisection of the sorted frame column, copies
//                         them to LDS with coalesced 8-byte loads (40-byte rows: nothing wider is aligned), and works on
//                         the copy.  A unit with more than EV_CAP rows on one side is read from memory in place by the
//                         same code.  Counters stay in registers; 16 + 1 atomics per wave at the end.
// The kernel is compiled for max_tracks <= 3 (every lane solves the cells of its class by enumeration, assign_3x3) and for
// max_tracks <= 8 (WIDE: a cell with 4 to 8 events on a side is handed to the whole wave, assign_wave_8x8; a cell with at
// most 3 on both sides still takes the enumeration, so it gives the same bits in both).
// seld_event_metrics_breakdown keeps the counters apart by recording and class: event_breakdown_kernel is
// event_metrics_kernel around the same score_unit (BY = true), every unit leaving a slab in a workspace instead of adding to
// the totals, and breakdown_reduce_kernel (metrics_common.h) adds the slabs of a recording in block order.
// least_distance_kernel solves a batch of associations alone (least_distance_between_gt_pred, Dcase21_metrics.py:191-220)
// with the same device functions.
#include "metrics_common.h"

namespace seld {

constexpr int EV_COUNTERS = 16;     // the 13 of metrics.hip | TP FP FN of sed_score_computation
constexpr int EV_CAP = 256;         // rows of one side of a unit staged in LDS (2 x 10 KB per wave)
constexpr int EV_WIDE = 8;          // SELD_EVENT_METRICS_MAX_TRACKS_EX: events of a cell assign_wave_8x8 takes

struct EventP {
    const double* pred;             // (pred_n, 2 + COORDS)
    const long long* pred_off;      // (recordings + 1)
    long long pred_n;
    const double* tru;
    const long long* true_off;
    long long true_n;
    long long recordings, blocks;
    int n_frames, classes, fpb, max_tracks;
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
template <int S, class Index>
__device__ __forceinline__ Index first_frame_not_below(const double* rows, Index lo, Index hi, double key) {
    while (lo < hi) {
        const Index mid = lo + (hi - lo) / 2;
        if (rows[mid * S] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool whole_in(double f, double lo, double hi) { return f >= lo && f < hi && f == floor(f); }

// the slab row of a list row's class: the class itself, or row "other" for one that is no integer in [0, classes)
__device__ __forceinline__ int class_row(double c, int classes) { return whole_in(c, 0.0, (double)classes) ? (int)c : classes; }

template <int COORDS>
__global__ __launch_bounds__(256) void event_check_kernel(const EventP p) {
    constexpr int S = 2 + COORDS;
    const int mt = p.max_tracks;
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
        const double f = rows[row * S], c = rows[row * S + 1];
        if (!whole_in(f, 0.0, (double)p.n_frames)) ++bad_frame;
        if (whole_in(f, 0.0, dcase_end) && whole_in(c, 0.0, (double)p.classes)) {
            int earlier = 0;                            // events of the same cell in front of this one
            for (long long j = row - 1; j >= lo && rows[j * S] == f && earlier <= mt; --j) earlier += rows[j * S + 1] == c ? 1 : 0;
            if (earlier == mt) ++bad_cell;              // event max_tracks + 1 of its cell: every overflowing cell has one
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
// COORDS = 2: the Euclidean counters cnt[0..2] have no meaning and are left alone.  WIDE: h and cs are the LDS of
// assign_wave_8x8.  BY: `slab` is the unit's zeroed LDS slab (metrics_common.h) and cnt / total_de hold this unit alone:
// whatever a row or a class adds to cnt goes into its class row of the slab as well.
template <int COORDS, bool WIDE, bool BY>
__device__ __forceinline__ void score_unit(const double* P, int np, const double* T, int nt, const EventP& p, double f0, int lane,
                                           long long (&cnt)[EV_COUNTERS], double& total_de, double* h, double* cs,
                                           long long* slab) {
    constexpr int S = 2 + COORDS;
    constexpr int NT = WIDE ? EV_WIDE : 3;              // reference tracks a class can have
    // ---- location_sensitive_detection and sed_score_computation: lane = row ----
    // Per frame: no reference -> FP += 2 p; no prediction -> FN += 2 t; else TP += m, FN += t - m, FP += p - m.  Row by
    // row that is: a prediction adds 1 to FP (2 where its frame has no reference), a reference adds 2 to FN where its
    // frame has no prediction, else TP + 1 and FP - 1 when matched, FN + 1 when not.  cnt[13..15] the same on the class alone.
    const double lsd_end = (double)p.n_frames;
    for (int i = lane; i < np; i += 64) {
        const double f = P[i * S];
        if (!whole_in(f, 0.0, lsd_end)) continue;
        const int j = first_frame_not_below<S>(T, 0, nt, f);
        const int add = (j < nt && T[j * S] == f) ? 1 : 2;
        if constexpr (COORDS == 3) cnt[1] += add;
        cnt[14] += add;
        if constexpr (BY) {
            const int row = class_row(P[i * S + 1], p.classes);
            if constexpr (COORDS == 3) slab_add(slab, row, 1, add);
            slab_add(slab, row, 14, add);
        }
    }
    for (int i = lane; i < nt; i += 64) {
        const double f = T[i * S];
        if (!whole_in(f, 0.0, lsd_end)) continue;
        int j = first_frame_not_below<S>(P, 0, np, f);
        if (!(j < np && P[j * S] == f)) {
            if constexpr (COORDS == 3) cnt[2] += 2;
            cnt[15] += 2;
            if constexpr (BY) {
                const int row = class_row(T[i * S + 1], p.classes);
                if constexpr (COORDS == 3) slab_add(slab, row, 2, 2);
                slab_add(slab, row, 15, 2);
            }
            continue;
        }
        const double c = T[i * S + 1];
        bool near = false, same = false;
        if constexpr (COORDS == 3) {
            const double x = T[i * S + 2], y = T[i * S + 3], z = T[i * S + 4];
            for (; j < np && P[j * S] == f; ++j) {
                if (P[j * S + 1] != c) continue;
                same = true;
                const double dx = x - P[j * S + 2], dy = y - P[j * S + 3], dz = z - P[j * S + 4];
                if (sqrt(dx * dx + dy * dy + dz * dz) < p.spatial_threshold) near = true;
            }
            cnt[0] += near ? 1 : 0;
            cnt[1] -= near ? 1 : 0;
            cnt[2] += near ? 0 : 1;
            if constexpr (BY) {
                const int row = class_row(c, p.classes);
                slab_add(slab, row, near ? 0 : 2, 1);
                if (near) slab_add(slab, row, 1, -1);
            }
        } else {
            for (; j < np && P[j * S] == f; ++j) same = same || P[j * S + 1] == c;
        }
        cnt[13] += same ? 1 : 0;
        cnt[14] -= same ? 1 : 0;
        cnt[15] += same ? 0 : 1;
        if constexpr (BY) {
            const int row = class_row(c, p.classes);
            slab_add(slab, row, same ? 13 : 15, 1);
            if (same) slab_add(slab, row, 14, -1);
        }
    }
    if (p.classes == 0) return;

    // ---- DCASE21 block metrics: lane = class ----
    // Every lane walks the two lists together, frame by frame in ascending order, and keeps the events of its own class:
    // up to 3 references g and 3 predictions q of the frame in registers (spherical ones turned into radians as they are
    // read), the longest list of each side, and per reference track the sum and count of its matched distances.
    const double mine = lane < p.classes ? (double)lane : __builtin_nan("");      // NaN equals no class
    int ip = 0, it = 0, nb_gt = 0, nb_pred = 0;
    int n[NT];
    double s[NT];
#pragma unroll
    for (int r = 0; r < NT; ++r) {
        n[r] = 0;
        s[r] = 0.0;
    }
    while (ip < np || it < nt) {
        const double fp = ip < np ? P[ip * S] : __builtin_inf(), ft = it < nt ? T[it * S] : __builtin_inf();
        if (fp != fp) { ++ip; continue; }               // a NaN frame belongs to no block: stepped over, wherever it sorts
        if (ft != ft) { ++it; continue; }
        const double f = fmin(fp, ft);
        const bool frame_ok = whole_in(f, f0, f0 + (double)p.fpb);
        double ga[3][COORDS], qa[3][COORDS];
        int g = 0, q = 0;
        const int it0 = it, ip0 = ip;                   // the frame's rows are [it0, it) and [ip0, ip) after the two loops
        for (; it < nt && !(T[it * S] > f); ++it) {      // not above: a NaN frame is stepped over, never waited for
            if (!(frame_ok && T[it * S] == f && T[it * S + 1] == mine)) continue;
#pragma unroll
            for (int e = 0; e < 3; ++e)
                if (g == e) {
#pragma unroll
                    for (int k = 0; k < COORDS; ++k) ga[e][k] = COORDS == 3 ? T[it * S + 2 + k] : deg_to_rad(T[it * S + 2 + k]);
                }
            ++g;
        }
        for (; ip < np && !(P[ip * S] > f); ++ip) {
            if (!(frame_ok && P[ip * S] == f && P[ip * S + 1] == mine)) continue;
#pragma unroll
            for (int e = 0; e < 3; ++e)
                if (q == e) {
#pragma unroll
                    for (int k = 0; k < COORDS; ++k) qa[e][k] = COORDS == 3 ? P[ip * S + 2 + k] : deg_to_rad(P[ip * S + 2 + k]);
                }
            ++q;
        }
        g = min(g, NT);                                 // a longer list is refused by event_check_kernel before this runs
        q = min(q, NT);
        nb_gt = max(nb_gt, g);
        nb_pred = max(nb_pred, q);
        const bool wide = WIDE && g && q && (g > 3 || q > 3);
        if (g && q && !wide) {
            double cost[9];
#pragma unroll
            for (int e = 0; e < 3; ++e)
#pragma unroll
                for (int e2 = 0; e2 < 3; ++e2) cost[e * 3 + e2] = (e < g && e2 < q) ? doa_distance_deg<COORDS>(ga[e], qa[e2]) : 0.0;
            double o0 = -1.0, o1 = -1.0, o2 = -1.0;
            assign_3x3((1u << g) - 1u, (1u << q) - 1u, cost, o0, o1, o2);
            if (o0 >= 0.0) { s[0] += o0; ++n[0]; }
            if (o1 >= 0.0) { s[1] += o1; ++n[1]; }
            if (o2 >= 0.0) { s[2] += o2; ++n[2]; }
        }
        if constexpr (WIDE) {
            // the classes whose cell of this frame is larger than 3 x 3, one after the other, each by the whole wave: lane
            // 8 i + j finds reference i and prediction j of the class among the frame's rows and brings their distance
            unsigned long long todo = __builtin_amdgcn_ballot_w64(wide);
            while (todo) {
                const int c = __ffsll((long long)todo) - 1;
                todo &= todo - 1ull;
                const int gc = __shfl(g, c, 64), qc = __shfl(q, c, 64);
                const int i = lane >> 3, j = lane & 7;
                const double cd = (double)c;
                int ti = -1, pj = -1, seen = 0;
                for (int r = it0; r < it; ++r) {
                    if (!(T[r * S] == f && T[r * S + 1] == cd)) continue;
                    ti = seen == i ? r : ti;
                    ++seen;
                }
                seen = 0;
                for (int r = ip0; r < ip; ++r) {
                    if (!(P[r * S] == f && P[r * S + 1] == cd)) continue;
                    pj = seen == j ? r : pj;
                    ++seen;
                }
                double d = 0.0;
                if (i < gc && j < qc && ti >= 0 && pj >= 0) {
                    double a[COORDS], b[COORDS];
#pragma unroll
                    for (int k = 0; k < COORDS; ++k) {
                        a[k] = COORDS == 3 ? T[ti * S + 2 + k] : deg_to_rad(T[ti * S + 2 + k]);
                        b[k] = COORDS == 3 ? P[pj * S + 2 + k] : deg_to_rad(P[pj * S + 2 + k]);
                    }
                    d = doa_distance_deg<COORDS>(a, b);
                }
                const int col = assign_wave_8x8(gc, qc, d, lane, h, cs);
#pragma unroll
                for (int r = 0; r < EV_WIDE; ++r) {
                    const int cr = __shfl(col, r, 64);                      // the column of reference track r
                    const double dr = __shfl(d, r * 8 + (cr & 7), 64);
                    if (lane == c && r < gc && cr < qc) {
                        s[r] += dr;
                        ++n[r];
                    }
                }
            }
        }
    }
    int loc_fn = 0, loc_fp = 0;
    if (lane < p.classes) {
        const DcaseAdd a = dcase_class_block_n<NT>(nb_gt, nb_pred, s, n, p.doa_threshold, total_de);
        SELD_DCASE_ADD(cnt, a);
        loc_fn = a.fn;
        loc_fp = a.fp;
        if constexpr (BY) slab_put_dcase(slab, lane, a, total_de);
    }
    const int blk_fn = wave_sum_i32(loc_fn), blk_fp = wave_sum_i32(loc_fp);
    if (lane == 0) {
        cnt[6] += min(blk_fp, blk_fn);
        cnt[7] += max(0, blk_fn - blk_fp);
        cnt[8] += max(0, blk_fp - blk_fn);
    }
}

template <int COORDS, bool WIDE>
__global__ __launch_bounds__(64) void event_metrics_kernel(const EventP p) {
    constexpr int S = 2 + COORDS;
    __shared__ __attribute__((aligned(16))) double pred_s[EV_CAP * S];
    __shared__ __attribute__((aligned(16))) double true_s[EV_CAP * S];
    double *h = nullptr, *cs = nullptr;
    if constexpr (WIDE) {                               // 2.5 KB more, in the instantiations that use it alone
        __shared__ double h_s[256], cs_s[64];
        h = h_s;
        cs = cs_s;
    }
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
        const long long p0 = first_frame_not_below<S>(p.pred, plo, phi, f0), p1 = first_frame_not_below<S>(p.pred, p0, phi, f1);
        const long long t0 = first_frame_not_below<S>(p.tru, tlo, thi, f0), t1 = first_frame_not_below<S>(p.tru, t0, thi, f1);
        const int np = (int)(p1 - p0), nt = (int)(t1 - t0);
        if (np == 0 && nt == 0) continue;
        if (np <= EV_CAP && nt <= EV_CAP) {
            for (int i = lane; i < np * S; i += 64) pred_s[i] = p.pred[p0 * S + i];
            for (int i = lane; i < nt * S; i += 64) true_s[i] = p.tru[t0 * S + i];
            __syncthreads();
            score_unit<COORDS, WIDE, false>(pred_s, np, true_s, nt, p, f0, lane, cnt, total_de, h, cs, nullptr);
            __syncthreads();                            // the copy is rewritten by the next unit
        } else {
            score_unit<COORDS, WIDE, false>(p.pred + p0 * S, np, p.tru + t0 * S, nt, p, f0, lane, cnt, total_de, h, cs, nullptr);
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

// event_metrics_kernel with the closing sums kept apart: every (recording, block) unit, an empty one too, leaves its
// slab (metrics_common.h) in p.work, and breakdown_reduce_kernel adds them up.  The scoring is score_unit's.
template <int COORDS, bool WIDE>
__global__ __launch_bounds__(64) void event_breakdown_kernel(const EventP p, long long* work) {
    constexpr int S = 2 + COORDS;
    __shared__ __attribute__((aligned(16))) double pred_s[EV_CAP * S];
    __shared__ __attribute__((aligned(16))) double true_s[EV_CAP * S];
    __shared__ long long slab[(64 + 2) * BY_ROW];
    double *h = nullptr, *cs = nullptr;
    if constexpr (WIDE) {
        __shared__ double h_s[256], cs_s[64];
        h = h_s;
        cs = cs_s;
    }
    if (p.flags[1] != 0) return;                        // refused: the reduction writes zeros and reads no slab
    const int lane = threadIdx.x;
    const int words = (p.classes + 2) * BY_ROW;
    const long long total = p.recordings * p.blocks;
    for (long long u = blockIdx.x; u < total; u += gridDim.x) {
        const long long rec = u / p.blocks, blk = u % p.blocks;
        const double f0 = (double)blk * (double)p.fpb, f1 = f0 + (double)p.fpb;
        long long plo = 0, phi = 0, tlo = 0, thi = 0;
        if (p.pred_n) rec_range(p.pred_off, rec, p.pred_n, plo, phi);
        if (p.true_n) rec_range(p.true_off, rec, p.true_n, tlo, thi);
        const long long p0 = first_frame_not_below<S>(p.pred, plo, phi, f0), p1 = first_frame_not_below<S>(p.pred, p0, phi, f1);
        const long long t0 = first_frame_not_below<S>(p.tru, tlo, thi, f0), t1 = first_frame_not_below<S>(p.tru, t0, thi, f1);
        const int np = (int)(p1 - p0), nt = (int)(t1 - t0);
        long long* dst = work + u * words;
        if (np == 0 && nt == 0) {
            for (int i = lane; i < words; i += 64) dst[i] = 0;      // (the bits of 0.0 as well)
            continue;
        }
        for (int i = lane; i < words; i += 64) slab[i] = 0;
        long long cnt[EV_COUNTERS];
#pragma unroll
        for (int i = 0; i < EV_COUNTERS; ++i) cnt[i] = 0;
        double total_de = 0.0;
        if (np <= EV_CAP && nt <= EV_CAP) {
            for (int i = lane; i < np * S; i += 64) pred_s[i] = p.pred[p0 * S + i];
            for (int i = lane; i < nt * S; i += 64) true_s[i] = p.tru[t0 * S + i];
            __syncthreads();
            score_unit<COORDS, WIDE, true>(pred_s, np, true_s, nt, p, f0, lane, cnt, total_de, h, cs, slab);
        } else {
            __syncthreads();
            score_unit<COORDS, WIDE, true>(p.pred + p0 * S, np, p.tru + t0 * S, nt, p, f0, lane, cnt, total_de, h, cs, slab);
        }
        slab_put_all(slab, p.classes + 1, lane, cnt, total_de);
        __syncthreads();
        for (int i = lane; i < words; i += 64) dst[i] = slab[i];
        __syncthreads();                                // the slab and the copy are rewritten by the next unit
    }
}

struct AssignP {
    const double *gt, *pred;        // (problems, 8, COORDS)
    const int *gt_n, *pred_n;
    long long problems;
    double* cost;                   // (problems, 8)
    int *row, *col, *pairs;         // (problems, 8) twice, (problems)
};

// One wave per problem at a time.  Counts are forced into [0, 8], so nothing outside the arrays is read.
template <int COORDS>
__global__ __launch_bounds__(64) void least_distance_kernel(const AssignP p) {
    __shared__ double h[256], cs[64];
    const int lane = threadIdx.x, i = lane >> 3, j = lane & 7;
    for (long long b = blockIdx.x; b < p.problems; b += gridDim.x) {
        const int g = min(max(p.gt_n[b], 0), EV_WIDE), q = min(max(p.pred_n[b], 0), EV_WIDE);
        double d = 0.0;
        if (i < g && j < q) d = doa_distance_deg<COORDS>(p.gt + (b * 8 + i) * COORDS, p.pred + (b * 8 + j) * COORDS);
        const int col = assign_wave_8x8(g, q, d, lane, h, cs);
        const bool on = lane < g && col < q;            // lane = reference; g <= 8
        const unsigned long long matched = __builtin_amdgcn_ballot_w64(on);
        const double mine = __shfl(d, j * 8 + (col & 7), 64);
        const int pairs = min(g, q);
        if (on) {                                       // rows ascending, as linear_sum_assignment returns them
            const int k = __popcll(matched & ((1ull << lane) - 1ull));
            p.cost[b * 8 + k] = mine;
            p.row[b * 8 + k] = lane;
            p.col[b * 8 + k] = col;
        }
        if (lane >= pairs && lane < 8) {
            p.cost[b * 8 + lane] = 0.0;
            p.row[b * 8 + lane] = -1;
            p.col[b * 8 + lane] = -1;
        }
        if (lane == 0) p.pairs[b] = pairs;
    }
}

}  // namespace seld

using namespace seld;

// The checks both scoring calls make before anything is launched, and the kernels' arguments (without the outputs)
static int event_args(const double* pred_rows, const int64_t* pred_offsets, int64_t pred_count, const double* true_rows,
                      const int64_t* true_offsets, int64_t true_count, int64_t recordings, int32_t n_frames, int32_t nb_classes,
                      int32_t frames_per_block, int32_t coords, int32_t max_tracks, double spatial_threshold,
                      double doa_threshold, const void* out0, const void* out1, int64_t* flags, EventP& p) {
    if ((coords != 2 && coords != 3) || max_tracks < 1 || max_tracks > EV_WIDE) return SELD_EINVAL;
    if (recordings < 0 || pred_count < 0 || true_count < 0 || n_frames < 0 || !out0 || !out1 || !flags) return SELD_EINVAL;
    if (nb_classes < 0 || nb_classes > 64 || frames_per_block < 1) return SELD_EINVAL;
    if (pred_count > 0x0fffffff || true_count > 0x0fffffff) return SELD_EUNSUPPORTED;    // stride * row index stays an int inside a unit
    if ((pred_count && (!pred_rows || !pred_offsets)) || (true_count && (!true_rows || !true_offsets))) return SELD_EINVAL;
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
    p.max_tracks = max_tracks;
    p.spatial_threshold = spatial_threshold;
    p.doa_threshold = doa_threshold;
    p.counters = nullptr;
    p.total_de = nullptr;
    p.flags = reinterpret_cast<long long*>(flags);
    return SELD_OK;
}

static int zero_flags(int64_t* flags, hipStream_t stream) {
    const hipError_t e = hipMemsetAsync(flags, 0, 2 * sizeof(int64_t), stream);
    if (e != hipSuccess) {
        g_last_hip_error = (int)e;
        return SELD_ELAUNCH;
    }
    return SELD_OK;
}

static int launch_event_check(const EventP& p, int32_t coords, hipStream_t stream) {
    long long wgs = (p.pred_n + p.true_n + 255) / 256;
    if (wgs > 2048) wgs = 2048;
    if (coords == 3) hipLaunchKernelGGL(event_check_kernel<3>, dim3((unsigned)wgs), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(event_check_kernel<2>, dim3((unsigned)wgs), dim3(256), 0, stream, p);
    return check_launch();
}

extern "C" int seld_event_metrics_accumulate_ex(const double* pred_rows, const int64_t* pred_offsets, int64_t pred_count,
                                                const double* true_rows, const int64_t* true_offsets, int64_t true_count,
                                                int64_t recordings, int32_t n_frames, int32_t nb_classes,
                                                int32_t frames_per_block, int32_t coords, int32_t max_tracks,
                                                double spatial_threshold, double doa_threshold, int64_t* counters,
                                                double* total_de, int64_t* flags, void* stream) {
    EventP p;
    int rc = event_args(pred_rows, pred_offsets, pred_count, true_rows, true_offsets, true_count, recordings, n_frames, nb_classes,
                        frames_per_block, coords, max_tracks, spatial_threshold, doa_threshold, counters, total_de, flags, p);
    if (rc != SELD_OK) return rc;
    rc = zero_flags(flags, (hipStream_t)stream);
    if (rc != SELD_OK) return rc;
    if (recordings == 0) return SELD_OK;
    p.counters = reinterpret_cast<long long*>(counters);
    p.total_de = total_de;
    if (pred_count + true_count == 0) return SELD_OK;   // nothing to check, and every unit is empty
    rc = launch_event_check(p, coords, (hipStream_t)stream);
    if (rc != SELD_OK) return rc;
    const long long total = recordings * p.blocks;
    if (total == 0) return SELD_OK;
    const long long wgs = total > 4096 ? 4096 : total;  // 2 generations of resident waves; waves loop over their units
    const bool wide = max_tracks > 3;                   // up to 3 x 3 keeps the lane-per-class kernel as it was
    const dim3 grid((unsigned)wgs), block(64);
    if (coords == 3 && !wide) hipLaunchKernelGGL((event_metrics_kernel<3, false>), grid, block, 0, (hipStream_t)stream, p);
    else if (coords == 3) hipLaunchKernelGGL((event_metrics_kernel<3, true>), grid, block, 0, (hipStream_t)stream, p);
    else if (!wide) hipLaunchKernelGGL((event_metrics_kernel<2, false>), grid, block, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL((event_metrics_kernel<2, true>), grid, block, 0, (hipStream_t)stream, p);
    return check_launch();
}

extern "C" size_t seld_metrics_breakdown_workspace(int64_t recordings, int32_t n_frames, int32_t nb_classes,
                                                   int32_t frames_per_block) {
    if (recordings < 0 || n_frames < 0 || nb_classes < 0 || nb_classes > 64 || frames_per_block < 1) return 0;
    return breakdown_workspace_bytes(recordings, ((long long)n_frames + frames_per_block - 1) / frames_per_block, nb_classes);
}

extern "C" int seld_event_metrics_breakdown(const double* pred_rows, const int64_t* pred_offsets, int64_t pred_count,
                                            const double* true_rows, const int64_t* true_offsets, int64_t true_count,
                                            int64_t recordings, int32_t n_frames, int32_t nb_classes, int32_t frames_per_block,
                                            int32_t coords, int32_t max_tracks, double spatial_threshold, double doa_threshold,
                                            int64_t* counters, double* total_de, void* workspace, size_t workspace_bytes,
                                            int64_t* flags, void* stream) {
    EventP p;
    int rc = event_args(pred_rows, pred_offsets, pred_count, true_rows, true_offsets, true_count, recordings, n_frames, nb_classes,
                        frames_per_block, coords, max_tracks, spatial_threshold, doa_threshold, counters, total_de, flags, p);
    if (rc != SELD_OK) return rc;
    const size_t need = breakdown_workspace_bytes(recordings, p.blocks, nb_classes);
    if (need && (!workspace || workspace_bytes < need)) return SELD_EWORKSPACE;
    rc = zero_flags(flags, (hipStream_t)stream);
    if (rc != SELD_OK) return rc;
    if (recordings == 0) return SELD_OK;
    BreakdownP b;
    b.work = reinterpret_cast<const long long*>(workspace);
    b.flags = p.flags;
    b.recordings = recordings;
    b.blocks = p.blocks;
    b.rows = nb_classes + 2;
    b.counters = reinterpret_cast<long long*>(counters);
    b.total_de = total_de;
    const long long total = recordings * p.blocks;
    if (pred_count + true_count == 0) b.blocks = 0;     // every unit is empty: the table is zeros, no slab is written or read
    else {
        rc = launch_event_check(p, coords, (hipStream_t)stream);
        if (rc != SELD_OK) return rc;
    }
    if (b.blocks) {
        const long long wgs = total > 4096 ? 4096 : total;
        const bool wide = max_tracks > 3;
        const dim3 grid((unsigned)wgs), block(64);
        long long* work = reinterpret_cast<long long*>(workspace);
        if (coords == 3 && !wide) hipLaunchKernelGGL((event_breakdown_kernel<3, false>), grid, block, 0, (hipStream_t)stream, p, work);
        else if (coords == 3) hipLaunchKernelGGL((event_breakdown_kernel<3, true>), grid, block, 0, (hipStream_t)stream, p, work);
        else if (!wide) hipLaunchKernelGGL((event_breakdown_kernel<2, false>), grid, block, 0, (hipStream_t)stream, p, work);
        else hipLaunchKernelGGL((event_breakdown_kernel<2, true>), grid, block, 0, (hipStream_t)stream, p, work);
        rc = check_launch();
        if (rc != SELD_OK) return rc;
    }
    return launch_breakdown_reduce(b, (hipStream_t)stream);
}

extern "C" int seld_event_metrics_accumulate(const double* pred_rows, const int64_t* pred_offsets, int64_t pred_count,
                                             const double* true_rows, const int64_t* true_offsets, int64_t true_count,
                                             int64_t recordings, int32_t n_frames, int32_t nb_classes, int32_t frames_per_block,
                                             double spatial_threshold, double doa_threshold, int64_t* counters,
                                             double* total_de, int64_t* flags, void* stream) {
    return seld_event_metrics_accumulate_ex(pred_rows, pred_offsets, pred_count, true_rows, true_offsets, true_count, recordings,
                                            n_frames, nb_classes, frames_per_block, 3, SELD_EVENT_METRICS_MAX_TRACKS,
                                            spatial_threshold, doa_threshold, counters, total_de, flags, stream);
}

extern "C" int seld_least_distance(const double* gt, const int32_t* gt_counts, const double* pred, const int32_t* pred_counts,
                                   int64_t problems, int32_t coords, double* cost, int32_t* row, int32_t* col, int32_t* pairs,
                                   void* stream) {
    if (problems < 0 || (coords != 2 && coords != 3)) return SELD_EINVAL;
    if (problems > 0x0fffffff) return SELD_EUNSUPPORTED;                                 // 8 * coords * problem index stays small
    if (problems == 0) return SELD_OK;
    if (!gt || !gt_counts || !pred || !pred_counts || !cost || !row || !col || !pairs) return SELD_EINVAL;
    AssignP p;
    p.gt = gt;
    p.pred = pred;
    p.gt_n = gt_counts;
    p.pred_n = pred_counts;
    p.problems = problems;
    p.cost = cost;
    p.row = row;
    p.col = col;
    p.pairs = pairs;
    const dim3 grid((unsigned)(problems > 4096 ? 4096 : problems)), block(64);
    if (coords == 3) hipLaunchKernelGGL(least_distance_kernel<3>, grid, block, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(least_distance_kernel<2>, grid, block, 0, (hipStream_t)stream, p);
    return check_launch();
}
