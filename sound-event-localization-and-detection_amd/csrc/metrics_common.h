// Device functions shared by the two metric kernel families: metrics.hip (dense network outputs) and event_metrics.hip
// (event rows).  Both compute the DCASE21 block metrics of Dcase21_metrics.py:51-154 with the code below, so a result
// cannot differ between them by more than the order of the final atomics.  The second half of the file is what their
// breakdowns by recording and class share: the slab a unit writes and the kernel that adds the slabs up.
#pragma once
#include "common.h"

namespace seld {

// Dcase21_metrics.py:171-188
__device__ __forceinline__ double angular_distance_deg(const double a[3], const double b[3]) {
#pragma clang fp contract(off)
    const double n1 = sqrt(((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]) + 1e-10);
    const double n2 = sqrt(((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]) + 1e-10);
    double d = ((a[0] / n1) * (b[0] / n2) + (a[1] / n1) * (b[1] / n2)) + (a[2] / n1) * (b[2] / n2);
    d = fmin(fmax(d, -1.0), 1.0);
    return acos(d) * 180.0 / 3.141592653589793;
}

// Dcase21_metrics.py:157-168 on {azimuth, elevation} in radians, operation by operation
__device__ __forceinline__ double spherical_distance_deg(const double a[2], const double b[2]) {
#pragma clang fp contract(off)
    double d = sin(a[1]) * sin(b[1]) + (cos(a[1]) * cos(b[1])) * cos(fabs(a[0] - b[0]));
    d = fmin(fmax(d, -1.0), 1.0);
    return acos(d) * 180.0 / 3.141592653589793;
}

// The distance of the reference's least_distance_between_gt_pred for DOAs of COORDS entries: 3 Cartesian, 2 spherical
template <int COORDS>
__device__ __forceinline__ double doa_distance_deg(const double* a, const double* b) {
    if constexpr (COORDS == 3) return angular_distance_deg(a, b);
    else return spherical_distance_deg(a, b);
}

// Dcase21_metrics.py:91-93: degrees to radians as `v * np.pi / 180.`
__device__ __forceinline__ double deg_to_rad(double v) {
#pragma clang fp contract(off)
    return v * 3.141592653589793 / 180.0;
}

__device__ __forceinline__ unsigned long long readlane_u64(unsigned long long v, int src_lane) {
    const unsigned lo = __builtin_amdgcn_readlane((unsigned)v, src_lane);
    const unsigned hi = __builtin_amdgcn_readlane((unsigned)(v >> 32), src_lane);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The Hungarian association of the <= 3 reference and <= 3 predicted DOAs of one class in one frame, by enumeration
// (first minimum in lexicographic order).  g_bits / p_bits: which of the 3 slots hold an event (both non-zero); cost
// [reference slot][predicted slot], read at present slots only.  o0 / o1 / o2 receive the matched distance of reference
// track 0 / 1 / 2 (the rank of the slot among the present references) and are left alone for an unmatched track.
// Everything is indexed with compile-time constants (registers, no scratch): absent slots are masked out of the
// enumeration instead of being compacted away.
__device__ __forceinline__ void assign_3x3(unsigned g_bits, unsigned p_bits, const double* cs, double& o0, double& o1,
                                           double& o2) {
    const int g = __popc(g_bits), q = __popc(p_bits);
    double cost[3][3];
#pragma unroll
    for (int e = 0; e < 3; ++e)
#pragma unroll
        for (int e2 = 0; e2 < 3; ++e2)
            cost[e][e2] = (((g_bits >> e) & 1u) && ((p_bits >> e2) & 1u)) ? cs[e * 3 + e2] : 0.0;
    // all 6 row -> column maps of the slots; a map counts when it pairs min(g, q) present rows with present
    // columns (a maximum matching); the cheapest one wins, the first on ties
    const int need = min(g, q);
    int best = -1;
    double best_cost = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        constexpr int P[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
        int pairs = 0;
        double tot = 0.0;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const bool on = ((g_bits >> e) & 1u) && ((p_bits >> P[k][e]) & 1u);
            pairs += on ? 1 : 0;
            tot += on ? cost[e][P[k][e]] : 0.0;
        }
        if (pairs == need && (best < 0 || tot < best_cost)) {
            best = k;
            best_cost = tot;
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        constexpr int P[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
        if (k != best) continue;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            if (!(((g_bits >> e) & 1u) && ((p_bits >> P[k][e]) & 1u))) continue;
            const int rank = __popc(g_bits & ((1u << e) - 1u));      // index of slot e among the present references
            const double d = cost[e][P[k][e]];
            o0 = rank == 0 ? d : o0;
            o1 = rank == 1 ? d : o1;
            o2 = rank == 2 ? d : o2;
        }
    }
}

// The association of g <= 8 reference with q <= 8 predicted DOAs by the whole wave of a ONE-WAVE workgroup (it uses the
// workgroup barrier).  Lane 8 i + j brings cost[i][j] (anything where i >= g or j >= q: it is replaced by 0); g and q
// are wave-uniform and either may be 0.  h (256 doubles) and cs (64 doubles) are LDS.  Returns, in lane r < 8,
// the column of row r: row r is matched when r < g and the column is below q.
//
// The problem is padded with zero-cost rows or columns to n x n, n = max(g, q): a perfect matching of the padded matrix
// costs what its min(g, q) real pairs cost.  h[mask] = the cheapest way to give rows n - popc(mask) .. n - 1 the columns
// of mask, filled layer by layer of popc(mask), four masks a lane; then rows 0, 1, ... each take the LOWEST column that
// keeps the optimum (cs[r][j] + h[mask ^ j] == h[mask], the very expression that produced h[mask]).  That is the first
// row -> column map in lexicographic order among the cheapest, an unmatched row counting as a column above every real
// one: assign_3x3's rule.  Sums are taken from the last row backwards.  No register array is indexed at run time.
__device__ __forceinline__ int assign_wave_8x8(int g, int q, double c, int lane, double* h, double* cs) {
#pragma clang fp contract(off)
    const int n = max(g, q);
    const unsigned full = (1u << n) - 1u;
    cs[lane] = ((lane >> 3) < g && (lane & 7) < q) ? c : 0.0;
    if (lane == 0) h[0] = 0.0;
    __syncthreads();
    for (int k = 1; k <= n; ++k) {
        const int r = n - k;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const unsigned m = (unsigned)lane + 64u * t;
            if (m > full || __popc(m) != k) continue;
            double best = __builtin_inf();
            for (unsigned rest = m; rest; rest &= rest - 1u) {
                const int j = __ffs(rest) - 1;
                const double v = cs[r * 8 + j] + h[m ^ (1u << j)];
                best = v < best ? v : best;
            }
            h[m] = best;
        }
        __syncthreads();
    }
    unsigned m = full;
    int mine = 8;
    for (int r = 0; r < n; ++r) {
        const double want = h[m];
        int pick = __ffs(m) - 1;                        // (only a NaN cost leaves the search below empty-handed)
        for (unsigned rest = m; rest; rest &= rest - 1u) {
            const int j = __ffs(rest) - 1;
            if (cs[r * 8 + j] + h[m ^ (1u << j)] == want) {
                pick = j;
                break;
            }
        }
        mine = lane == r ? pick : mine;
        m ^= 1u << pick;
    }
    __syncthreads();                                    // h and cs are rewritten by the next problem
    return mine;
}

// What one class of one block adds to the DCASE21 counters (Dcase21_metrics.py:65-149).  fp and fn are also the class's
// share of the block's loc_FP and loc_FN, which the reference raises wherever it raises _FP and _FN.
struct DcaseAdd {
    int tp, fp, fn, nref, de_tp, de_fp, de_fn;
};

// nb_gt / nb_pred: the longest reference / predicted list of a frame of the block; s / n: the sum and the count of the
// matched distances of reference track 0 .. N - 1 over the block's frames.  The tracks' averages are added to total_de
// in track order.
template <int N>
__device__ __forceinline__ DcaseAdd dcase_class_block_n(int nb_gt, int nb_pred, const double (&s)[N], const int (&n)[N],
                                                        double doa_threshold, double& total_de) {
    DcaseAdd a = {0, 0, 0, nb_gt, 0, 0, 0};
    if (nb_gt && nb_pred) {
        int matched = 0;
#pragma unroll
        for (int r = 0; r < N; ++r) matched += n[r];
        if (matched == 0) {
            a.fn += nb_pred;
            a.de_fn += nb_pred;
        } else {
            // (the reference adds the tracks' averages in order of first appearance; the order only moves the last
            //  bit of _total_DE, which the cross-block atomics reorder anyway)
#pragma unroll
            for (int r = 0; r < N; ++r) {
                if (n[r] == 0) continue;
                const double avg = s[r] / (double)n[r];
                total_de += avg;
                a.de_tp += 1;
                if (avg <= doa_threshold) a.tp += 1; else a.fp += 1;
            }
            if (nb_pred > nb_gt) {
                a.fp += nb_pred - nb_gt;
                a.de_fp += nb_pred - nb_gt;
            } else if (nb_pred < nb_gt) {
                a.fn += nb_gt - nb_pred;
                a.de_fn += nb_gt - nb_pred;
            }
        }
    } else if (nb_gt) {
        a.fn += nb_gt;
        a.de_fn += nb_gt;
    } else if (nb_pred) {
        a.fp += nb_pred;
        a.de_fp += nb_pred;
    }
    return a;
}

__device__ __forceinline__ DcaseAdd dcase_class_block(int nb_gt, int nb_pred, double s0, double s1, double s2, int n0, int n1,
                                                      int n2, double doa_threshold, double& total_de) {
    const double s[3] = {s0, s1, s2};
    const int n[3] = {n0, n1, n2};
    return dcase_class_block_n<3>(nb_gt, nb_pred, s, n, doa_threshold, total_de);
}

// cnt: the counters in METRIC_COUNTERS order
#define SELD_DCASE_ADD(cnt, a) \
    do { \
        cnt[3] += (a).tp; cnt[4] += (a).fp; cnt[5] += (a).fn; cnt[9] += (a).nref; \
        cnt[10] += (a).de_tp; cnt[11] += (a).de_fp; cnt[12] += (a).de_fn; \
    } while (0)

// ---- the breakdown by recording and class (seld_event_metrics_breakdown, seld_metrics_breakdown) ----
// A slab is what one (recording, block) unit adds, one row per class, then "other", then "all": BY_ROW 8-byte words a
// row, the 16 counters in EVENT_METRIC_COUNTERS order and the row's total_DE as a double.  A wave builds the slab of its
// unit in LDS (rows of classes with LDS integer atomics for the detection counters, whose lanes are list rows; plain
// stores by the class's own lane for the DCASE counters), copies it to slab `unit` of the workspace, and
// breakdown_reduce_kernel adds the slabs of a recording in block order: no global atomics, nothing to zero beforehand,
// the same bits every run.
constexpr int BY_COUNTERS = 16;
constexpr int BY_ROW = BY_COUNTERS + 1;

inline size_t breakdown_workspace_bytes(long long recordings, long long blocks, int classes) {
    return (size_t)recordings * (size_t)blocks * (size_t)(classes + 2) * BY_ROW * sizeof(long long);
}

// one more count in counter k of class row `row` of the LDS slab (v may be negative)
__device__ __forceinline__ void slab_add(long long* slab, int row, int k, int v) {
    atomicAdd(reinterpret_cast<unsigned long long*>(slab + row * BY_ROW + k), (unsigned long long)(long long)v);
}

// what class `row` of one block adds to the DCASE counters, by the row's own lane; S, D, I from the class's own
// loc_FP / loc_FN (the class-wise definition behind DCASE's macro average)
__device__ __forceinline__ void slab_put_dcase(long long* slab, int row, const DcaseAdd& a, double de) {
    long long* s = slab + row * BY_ROW;
    s[3] = a.tp; s[4] = a.fp; s[5] = a.fn;
    s[6] = min(a.fp, a.fn); s[7] = max(0, a.fn - a.fp); s[8] = max(0, a.fp - a.fn);
    s[9] = a.nref; s[10] = a.de_tp; s[11] = a.de_fp; s[12] = a.de_fn;
    reinterpret_cast<double*>(s)[BY_COUNTERS] = de;
}

// row "all" of the slab: the wave's sums of what the unit added to the lanes' counters, which is what the plain call adds
template <int N>
__device__ __forceinline__ void slab_put_all(long long* slab, int row, int lane, const long long (&cnt)[N], double total_de) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const long long s = wave_sum_i64(cnt[i]);
        if (lane == 0) slab[row * BY_ROW + i] = s;
    }
    const double de = wave_sum_d(total_de);
    if (lane == 0) reinterpret_cast<double*>(slab)[row * BY_ROW + BY_COUNTERS] = de;
}

struct BreakdownP {
    const long long* work;          // (recordings, blocks, rows, BY_ROW) slabs
    const long long* flags;         // flags[1] != 0: a refused call, the table is zeros (NULL: never refused)
    long long recordings, blocks;
    int rows;                       // classes + 2
    long long* counters;            // (recordings, rows, 16)
    double* total_de;               // (recordings, rows)
};

// One thread per word of the table; the blocks of its recording in ascending order.  Neighbouring threads read
// neighbouring words of a slab.
template <int ROW>
__global__ __launch_bounds__(256) void breakdown_reduce_kernel(const BreakdownP p) {
    const long long words = p.recordings * p.rows * ROW;
    const bool refused = p.flags && p.flags[1] != 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (long long)gridDim.x * blockDim.x) {
        const long long rec = i / ((long long)p.rows * ROW);
        const int w = (int)(i - rec * p.rows * ROW), row = w / ROW, k = w - row * ROW;
        const long long* src = p.work + rec * p.blocks * p.rows * ROW + w;
        if (k < ROW - 1) {
            long long s = 0;
            if (!refused)
                for (long long b = 0; b < p.blocks; ++b) s += src[b * p.rows * ROW];
            p.counters[(rec * p.rows + row) * (ROW - 1) + k] = s;
        } else {
            double s = 0.0;
            if (!refused)
                for (long long b = 0; b < p.blocks; ++b) s += reinterpret_cast<const double*>(src)[b * p.rows * ROW];
            p.total_de[rec * p.rows + row] = s;
        }
    }
}

inline int launch_breakdown_reduce(const BreakdownP& p, hipStream_t stream) {
    const long long words = p.recordings * p.rows * BY_ROW;
    if (words == 0) return SELD_OK;
    long long wgs = (words + 255) / 256;
    if (wgs > 4096) wgs = 4096;
    hipLaunchKernelGGL(breakdown_reduce_kernel<BY_ROW>, dim3((unsigned)wgs), dim3(256), 0, stream, p);
    return check_launch();
}

}  // namespace seld
