// Element-wise quaternion algebra, gfx950: get_modulus / get_normalized / hamilton_product of quaternion_ops.py and
// dual_quaternion_ops.py, and q_normalize / quaternion_exp of dual_quaternion_ops.py (reference :88-108, :206-243,
// :374-412).  Exact fp32 on the VALU, forward and first derivatives.  The reference runs each as 10 to 40 ATen launches
// that copy the tensor several times; here each is ONE pass over memory (the batch-summed forms: one pass + a small fold).
//
// One index map serves every rank.  A contiguous input (dim0, mid, comp, inner) with the component axis `comp` = 4Q is
// the array (R, S, 4, M):  R = dim0,  S = mid,  M = Q * inner contiguous, component c of quaternion (r, s, m) at
//     in(r, s, c, m) = ((r*S + s)*4 + c)*M + m
//   2-D (N, 4Q):             R = N, S = 1, M = Q         3-D (B, T, 4Q): R = B, S = T, M = Q
//   4-D / 5-D (N, 4Q, ...):  R = N, S = 1, M = Q * prod(spatial)
// q_normalize and quaternion_exp concatenate their result on dim 1 whatever the rank: for a 3-D input that is
// (B, 4T, Q), i.e. (R, 4, S, M), SELD_QUAT_LAYOUT_CAT1:
//     out(r, c, s, m) = ((r*4 + c)*S + s)*M + m              (equal to in() when S = 1)
// The kernels read with in() and write (or read the cotangent) with out(): no permuted copy is ever made.
// Per-quaternion results (vector-form modulus) live at row(r, s, m) = (r*S + s)*M + m; results summed over dim 0
// (the default get_modulus, the divisor of get_normalized) at col(s, m) = s*M + m.
//
// A thread owns W consecutive m of one (r, s): W = 4 with 16-byte loads and stores when M % 4 == 0 and every pointer is
// 16-byte aligned (then every in / out / row / col offset is a multiple of 4), else W = 1.  The grid is capped and
// grid-strided.  sqrtf, expf, sincosf and the divisions are the correctly rounded / full-range forms.
//
// Sums over dim 0 (R): workgroups of TX x TY threads, TX threads across col, TY down R; workgroup (p, b) adds the rows
// of slice p for its TX*W columns -- each thread its rows in order, then the TY threads of a column in order through
// LDS -- and writes one partial per column to the workspace; the fold kernel adds the P partials of a column in a fixed
// order (and takes the root).  No float atomics: every result is run-to-run bit-identical, with or without
// SELD_DETERMINISTIC.
//
// A zero quaternion: every forward value is finite (modulus 0, q_normalize 0, quaternion_exp exp(r)*[cos 1e-4, 0, 0, 0]).
// Where the reference's autograd divides 0 by 0 the kernels use the factor 0: the vector-form modulus gradient is 0 at
// |q| = 0, the batch-summed modulus and get_normalized gradients drop the x / modulus term where the summed modulus is 0,
// and quaternion_exp's gradient keeps only exp(r) * dy_a * sin(n) / n for its i, j, k inputs at i = j = k = 0.
#include <algorithm>
#include <initializer_list>
#include "common.h"

namespace seld {

constexpr int QA_MAX_BLOCKS = 2048;            // 256 CUs x 8 workgroups, the rest is grid-strided
constexpr int QA_ROWS_PER_THREAD = 8;          // rows of dim 0 a reduction thread adds before the LDS step
constexpr int QA_MAX_PARTIAL_BLOCKS = 4096;

enum {
    QA_MODV, QA_MODV_BWD, QA_UNIT, QA_UNIT_BWD, QA_EXP, QA_EXP_BWD, QA_HPROD, QA_HPROD_BWD,
    QA_NORMALIZED, QA_NORMALIZED_BWD, QA_MODS_BWD
};

struct QaP {
    int R, S, M;
    int cat1;                 // the quaternion-layout result / cotangent is (R, 4, S, M)
    unsigned items;           // R * S * (M / W)
    float eps;
    const float* x;           // the input (q0 of the product)
    const float* x1;          // q1
    const float* dy;
    const float* u;           // (S, M): the summed modulus
    const float* v;           // (S, M): sum over dim 0 and the components of dy * x
    float* o0;
    float* o1;
};

template <int W>
struct QaV {
    float v[W];
};

template <int W>
__device__ __forceinline__ QaV<W> qa_ld(const float* __restrict__ p) {
    QaV<W> r;
    if constexpr (W == 4) {
        const float4 t = *(const float4*)p;
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else {
        r.v[0] = *p;
    }
    return r;
}

template <int W>
__device__ __forceinline__ void qa_st(float* __restrict__ p, const QaV<W>& r) {
    if constexpr (W == 4) *(float4*)p = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else *p = r.v[0];
}

// the offsets of item `it` (see the file comment); cs: component stride of the out() layout
struct QaIdx {
    long long in, out, row, col, cs;
};

template <int W>
__device__ __forceinline__ QaIdx qa_index(const QaP& p, unsigned it) {
    const unsigned mw = (unsigned)p.M / W;
    const unsigned o = it / mw, m = (it - o * mw) * W;
    const unsigned r = p.S == 1 ? o : o / (unsigned)p.S, s = o - r * (unsigned)p.S;
    QaIdx i;
    i.in = (long long)o * 4 * p.M + m;
    i.row = (long long)o * p.M + m;
    i.col = (long long)s * p.M + m;
    if (p.cat1) {
        i.cs = (long long)p.S * p.M;
        i.out = ((long long)r * 4 * p.S + s) * p.M + m;
    } else {
        i.cs = p.M;
        i.out = i.in;
    }
    return i;
}

// y = a (x) b, the Hamilton product (sign table: reference hamilton_product docstring)
__device__ __forceinline__ void qa_mul(const float a[4], const float b[4], float y[4]) {
    y[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    y[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    y[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    y[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
}

// One quaternion of op OP.  x: the input; b: q1 (product) ; g: the cotangent's components, or g[0] the per-quaternion /
// per-column cotangent; u, v: the per-column scalars.  Results in y (and y1: dq1).
template <int OP>
__device__ __forceinline__ void qa_one(const float x[4], const float b[4], const float g[4], float u, float v, float eps,
                                       float y[4], float y1[4]) {
    const float ss = x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3];
    if constexpr (OP == QA_MODV) {
        y[0] = sqrtf(ss);
    } else if constexpr (OP == QA_MODV_BWD) {
        const float f = ss > 0.f ? g[0] / sqrtf(ss) : 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) y[c] = x[c] * f;
    } else if constexpr (OP == QA_UNIT) {
        const float n = sqrtf(ss + 1e-4f);
#pragma unroll
        for (int c = 0; c < 4; ++c) y[c] = x[c] / n;
    } else if constexpr (OP == QA_UNIT_BWD) {
        const float n = sqrtf(ss + 1e-4f), inv = 1.0f / n;
        const float dot = g[0] * x[0] + g[1] * x[1] + g[2] * x[2] + g[3] * x[3];
        const float k = dot * inv * inv;
#pragma unroll
        for (int c = 0; c < 4; ++c) y[c] = (g[c] - x[c] * k) * inv;
    } else if constexpr (OP == QA_EXP || OP == QA_EXP_BWD) {
        const float m0 = sqrtf(x[1] * x[1] + x[2] * x[2] + x[3] * x[3]);
        const float n = m0 + 1e-4f;
        const float e = expf(x[0]);
        float sn, cs;
        sincosf(n, &sn, &cs);
        const float gn = sn / n;                             // sin(n) / n
        if constexpr (OP == QA_EXP) {
            y[0] = e * cs;
#pragma unroll
            for (int c = 1; c < 4; ++c) y[c] = e * (x[c] * gn);
        } else {
            // d/dr: the result itself.  d/dv_a = e * [dy_a * gn + (v_a / m0) * (-dy_0 * sin n + gn' * sum_b dy_b v_b)],
            // gn' = (n cos n - sin n) / n^2; v_a / m0 is taken as 0 at v = 0
            const float dv = g[1] * x[1] + g[2] * x[2] + g[3] * x[3];
            const float gp = (n * cs - sn) / (n * n);
            const float t = m0 > 0.f ? (gp * dv - g[0] * sn) / m0 : 0.f;
            y[0] = e * (g[0] * cs + gn * dv);
#pragma unroll
            for (int c = 1; c < 4; ++c) y[c] = e * (g[c] * gn + x[c] * t);
        }
    } else if constexpr (OP == QA_HPROD) {
        qa_mul(x, b, y);
    } else if constexpr (OP == QA_HPROD_BWD) {
        const float bc[4] = {b[0], -b[1], -b[2], -b[3]};
        const float xc[4] = {x[0], -x[1], -x[2], -x[3]};
        qa_mul(g, bc, y);                                    // dq0 = dy (x) conj(q1)
        qa_mul(xc, g, y1);                                   // dq1 = conj(q0) (x) dy
    } else if constexpr (OP == QA_NORMALIZED) {
        const float d = u + eps;
#pragma unroll
        for (int c = 0; c < 4; ++c) y[c] = x[c] / d;
    } else if constexpr (OP == QA_NORMALIZED_BWD) {
        // y = x / (D + eps), D = sqrt(sum over dim 0 and components of x^2):  dx = dy / (D + eps) - x * G / ((D + eps)^2 D)
        const float inv = 1.0f / (u + eps);
        const float k = u > 0.f ? v * inv * inv / u : 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) y[c] = g[c] * inv - x[c] * k;
    } else if constexpr (OP == QA_MODS_BWD) {
        const float f = u > 0.f ? g[0] / u : 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) y[c] = x[c] * f;
    }
}

template <int OP, int W>
__global__ __launch_bounds__(256) void quat_pointwise_kernel(const QaP p) {
    constexpr bool HAS_B = OP == QA_HPROD || OP == QA_HPROD_BWD;
    constexpr bool DY4 = OP == QA_UNIT_BWD || OP == QA_EXP_BWD || OP == QA_HPROD_BWD || OP == QA_NORMALIZED_BWD;
    constexpr bool OUT1 = OP == QA_MODV;                     // one result per quaternion
    constexpr bool CATIN = OP == QA_UNIT_BWD || OP == QA_EXP_BWD;   // the cotangent has the out() layout
    constexpr bool CATOUT = OP == QA_UNIT || OP == QA_EXP;
    constexpr bool COLS = OP == QA_NORMALIZED || OP == QA_NORMALIZED_BWD || OP == QA_MODS_BWD;
    const unsigned stride = gridDim.x * 256u;
    for (unsigned it = blockIdx.x * 256u + threadIdx.x; it < p.items; it += stride) {
        const QaIdx i = qa_index<W>(p, it);
        QaV<W> x[4], b[4], g[4], u, v, y[4], y1[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) x[c] = qa_ld<W>(p.x + i.in + (long long)c * p.M);
        if constexpr (HAS_B) {
#pragma unroll
            for (int c = 0; c < 4; ++c) b[c] = qa_ld<W>(p.x1 + i.in + (long long)c * p.M);
        }
        if constexpr (DY4) {
#pragma unroll
            for (int c = 0; c < 4; ++c) g[c] = qa_ld<W>(p.dy + (CATIN ? i.out + c * i.cs : i.in + (long long)c * p.M));
        } else if constexpr (OP == QA_MODV_BWD) {
            g[0] = qa_ld<W>(p.dy + i.row);
        } else if constexpr (OP == QA_MODS_BWD) {
            g[0] = qa_ld<W>(p.dy + i.col);
        }
        if constexpr (COLS) u = qa_ld<W>(p.u + i.col);
        if constexpr (OP == QA_NORMALIZED_BWD) v = qa_ld<W>(p.v + i.col);
#pragma unroll
        for (int l = 0; l < W; ++l) {
            float xs[4], bs[4] = {0.f, 0.f, 0.f, 0.f}, gs[4] = {0.f, 0.f, 0.f, 0.f}, ys[4], y1s[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                xs[c] = x[c].v[l];
                if constexpr (HAS_B) bs[c] = b[c].v[l];
                if constexpr (DY4) gs[c] = g[c].v[l];
            }
            if constexpr (OP == QA_MODV_BWD || OP == QA_MODS_BWD) gs[0] = g[0].v[l];
            qa_one<OP>(xs, bs, gs, COLS ? u.v[l] : 0.f, OP == QA_NORMALIZED_BWD ? v.v[l] : 0.f, p.eps, ys, y1s);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c == 0 || !OUT1) y[c].v[l] = ys[c];
                if constexpr (OP == QA_HPROD_BWD) y1[c].v[l] = y1s[c];
            }
        }
        if constexpr (OUT1) {
            qa_st<W>(p.o0 + i.row, y[0]);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                qa_st<W>(p.o0 + (CATOUT ? i.out + c * i.cs : i.in + (long long)c * p.M), y[c]);
                if constexpr (OP == QA_HPROD_BWD) qa_st<W>(p.o1 + i.in + (long long)c * p.M, y1[c]);
            }
        }
    }
}

// ---- sums over dim 0 -------------------------------------------------------------------------------------------------
struct QaRed {
    int txlog;                // TX = 1 << txlog threads across col, TY = 256 / TX down dim 0
    int bj;                   // workgroups across col
    int rpb;                  // rows of dim 0 per workgroup
    int P;                    // partials per column
};

// partial[p][col] = sum over the rows r of slice p and the four components of x^2 (DOT: of dy * x)
template <bool DOT, int W>
__global__ __launch_bounds__(256) void quat_reduce_partial_kernel(const QaP p, const QaRed q, float* __restrict__ ws) {
    __shared__ float red[256 * W];
    const int TX = 1 << q.txlog, TY = 256 >> q.txlog;
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> q.txlog;
    const int b = blockIdx.x % q.bj, pb = blockIdx.x / q.bj;
    const long long J = (long long)p.S * p.M;
    const long long j = ((long long)b * TX + tx) * W;
    float acc[W];
#pragma unroll
    for (int l = 0; l < W; ++l) acc[l] = 0.f;
    if (j < J) {
        const int s = (int)(j / p.M), m = (int)(j - (long long)s * p.M);
        const int r1 = min(p.R, (pb + 1) * q.rpb);
#pragma unroll 2
        for (int r = pb * q.rpb + ty; r < r1; r += TY) {
            const long long in = ((long long)r * p.S + s) * 4 * p.M + m;
            QaV<W> x[4], g[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                x[c] = qa_ld<W>(p.x + in + (long long)c * p.M);
                if constexpr (DOT) g[c] = qa_ld<W>(p.dy + in + (long long)c * p.M);
            }
#pragma unroll
            for (int l = 0; l < W; ++l) {
                float t = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) t += x[c].v[l] * (DOT ? g[c].v[l] : x[c].v[l]);
                acc[l] += t;
            }
        }
    }
    if (TY > 1) {
#pragma unroll
        for (int l = 0; l < W; ++l) red[(ty * TX + tx) * W + l] = acc[l];
        __syncthreads();
        if (ty == 0) {
            for (int k = 1; k < TY; ++k) {
#pragma unroll
                for (int l = 0; l < W; ++l) acc[l] += red[(k * TX + tx) * W + l];
            }
        }
    }
    if (ty == 0 && j < J) {
        QaV<W> o;
#pragma unroll
        for (int l = 0; l < W; ++l) o.v[l] = acc[l];
        qa_st<W>(ws + (long long)pb * J + j, o);
    }
}

// out[col] = sum_p partial[p][col] in a fixed order (ROOT: its square root); TX threads across col, TY across p
template <bool ROOT>
__global__ __launch_bounds__(256) void quat_reduce_fold_kernel(const float* __restrict__ ws, int P, long long J, int txlog,
                                                               float* __restrict__ out) {
    __shared__ float red[256];
    const int TX = 1 << txlog, TY = 256 >> txlog;
    const int tx = threadIdx.x & (TX - 1), ty = threadIdx.x >> txlog;
    const long long j = (long long)blockIdx.x * TX + tx;
    float acc = 0.f;
    if (j < J) {
#pragma unroll 4
        for (int k = ty; k < P; k += TY) acc += ws[(long long)k * J + j];
    }
    if (TY > 1) {
        red[ty * TX + tx] = acc;
        __syncthreads();
        if (ty == 0)
            for (int k = 1; k < TY; ++k) acc += red[k * TX + tx];
    }
    if (ty == 0 && j < J) out[j] = ROOT ? sqrtf(acc) : acc;
}

// ---- host side -------------------------------------------------------------------------------------------------------
static int qa_shape(const seld_quat_shape* s, QaP* p) {
    if (!s || s->dim0 < 1 || s->mid < 1 || s->comp < 4 || s->inner < 1 || s->comp % 4 != 0) return SELD_EINVAL;
    const long long M = (long long)(s->comp / 4) * s->inner;
    // the item index is 32-bit (one item: one quaternion, or four with 16-byte accesses)
    if (M >= (1LL << 31) || (long long)s->dim0 * s->mid * M >= (1LL << 31)) return SELD_EUNSUPPORTED;
    *p = QaP{};
    p->R = s->dim0;
    p->S = s->mid;
    p->M = (int)M;
    return SELD_OK;
}

static bool qa_aligned(std::initializer_list<const void*> ptrs) {
    for (const void* q : ptrs)
        if ((uintptr_t)q & 15) return false;
    return true;
}

template <int OP>
static int qa_pointwise(QaP& p, bool vec, hipStream_t st) {
    const int W = vec ? 4 : 1;
    p.items = (unsigned)((long long)p.R * p.S * (p.M / W));
    const unsigned blocks = (unsigned)std::min<long long>(((long long)p.items + 255) / 256, QA_MAX_BLOCKS);
    if (vec) hipLaunchKernelGGL((quat_pointwise_kernel<OP, 4>), dim3(blocks), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((quat_pointwise_kernel<OP, 1>), dim3(blocks), dim3(256), 0, st, p);
    return check_launch();
}

static int qa_log2_ceil(long long n) {
    int l = 0;
    while ((1LL << l) < n) ++l;
    return l;
}

// the split of a sum over dim 0 depends on the extents and W alone
static QaRed qa_red_plan(const QaP& p, int W) {
    QaRed q;
    const long long JT = (long long)p.S * p.M / W;
    q.txlog = std::min(8, qa_log2_ceil(JT));
    const int TX = 1 << q.txlog, TY = 256 >> q.txlog;
    const long long bj = (JT + TX - 1) / TX;
    long long rpb = (long long)TY * QA_ROWS_PER_THREAD;
    long long P = (p.R + rpb - 1) / rpb;
    const long long cap = std::max<long long>(1, QA_MAX_PARTIAL_BLOCKS / bj);
    if (P > cap) {
        rpb = ((p.R + cap - 1) / cap + TY - 1) / TY * TY;
        P = (p.R + rpb - 1) / rpb;
    }
    q.bj = (int)bj;
    q.rpb = (int)rpb;
    q.P = (int)P;
    return q;
}

// floats: the partials (the larger of the W = 4 and W = 1 splits) + one row for the folded sum
static long long qa_red_floats(const QaP& p) {
    const long long J = (long long)p.S * p.M;
    long long P = qa_red_plan(p, 1).P;
    if (p.M % 4 == 0) P = std::max<long long>(P, qa_red_plan(p, 4).P);
    return (P + 1) * J;
}

static int qa_red_check(const QaP& p) {
    // the workgroup index of both reduction kernels is 32-bit
    const long long J = (long long)p.S * p.M;
    const QaRed q = qa_red_plan(p, 1);
    if ((long long)q.bj * q.P >= (1LL << 31) || J >= (1LL << 31)) return SELD_EUNSUPPORTED;
    return SELD_OK;
}

// out[col] = (ROOT: sqrt of) the sum over dim 0 and the components of x^2 (DOT: of dy * x)
template <bool DOT, bool ROOT>
static int qa_reduce(const QaP& p, bool vec, float* ws, float* out, hipStream_t st) {
    const QaRed q = qa_red_plan(p, vec ? 4 : 1);
    const long long J = (long long)p.S * p.M;
    const dim3 grid((unsigned)((long long)q.bj * q.P)), blk(256);
    if (vec) hipLaunchKernelGGL((quat_reduce_partial_kernel<DOT, 4>), grid, blk, 0, st, p, q, ws);
    else hipLaunchKernelGGL((quat_reduce_partial_kernel<DOT, 1>), grid, blk, 0, st, p, q, ws);
    int rc = check_launch();
    if (rc) return rc;
    const int txlog = 8 - std::min(4, qa_log2_ceil(q.P));
    const unsigned fg = (unsigned)((J + (1 << txlog) - 1) >> txlog);
    hipLaunchKernelGGL((quat_reduce_fold_kernel<ROOT>), dim3(fg), blk, 0, st, (const float*)ws, q.P, J, txlog, out);
    return check_launch();
}

}  // namespace seld

using namespace seld;

#define QA_BEGIN(shape)                     \
    QaP p;                                  \
    {                                       \
        const int rc_ = qa_shape(shape, &p); \
        if (rc_) return rc_;                \
    }

extern "C" int seld_quat_modulus_fwd(const seld_quat_shape* shape, const float* x, float* y, void* stream) {
    QA_BEGIN(shape);
    if (!x || !y) return SELD_EINVAL;
    p.x = x; p.o0 = y;
    return qa_pointwise<QA_MODV>(p, p.M % 4 == 0 && qa_aligned({x, y}), (hipStream_t)stream);
}

extern "C" int seld_quat_modulus_bwd(const seld_quat_shape* shape, const float* x, const float* dy, float* dx, void* stream) {
    QA_BEGIN(shape);
    if (!x || !dy || !dx) return SELD_EINVAL;
    p.x = x; p.dy = dy; p.o0 = dx;
    return qa_pointwise<QA_MODV_BWD>(p, p.M % 4 == 0 && qa_aligned({x, dy, dx}), (hipStream_t)stream);
}

extern "C" size_t seld_quat_reduce_workspace(const seld_quat_shape* shape) {
    QaP p;
    if (qa_shape(shape, &p) != SELD_OK || qa_red_check(p) != SELD_OK) return 0;
    return (size_t)qa_red_floats(p) * sizeof(float);
}

extern "C" int seld_quat_modulus_sum_fwd(const seld_quat_shape* shape, const float* x, float* y, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    QA_BEGIN(shape);
    const int rc = qa_red_check(p);
    if (rc) return rc;
    if (!x || !y) return SELD_EINVAL;
    if (!workspace || workspace_bytes < (size_t)qa_red_floats(p) * sizeof(float)) return SELD_EWORKSPACE;
    p.x = x;
    return qa_reduce<false, true>(p, p.M % 4 == 0 && qa_aligned({x, workspace}), (float*)workspace, y, (hipStream_t)stream);
}

extern "C" int seld_quat_modulus_sum_bwd(const seld_quat_shape* shape, const float* x, const float* y, const float* dy,
                                         float* dx, void* stream) {
    QA_BEGIN(shape);
    if (!x || !y || !dy || !dx) return SELD_EINVAL;
    p.x = x; p.u = y; p.dy = dy; p.o0 = dx;
    return qa_pointwise<QA_MODS_BWD>(p, p.M % 4 == 0 && qa_aligned({x, y, dy, dx}), (hipStream_t)stream);
}

extern "C" int seld_quat_normalized_fwd(const seld_quat_shape* shape, const float* x, const float* modulus, float eps,
                                        float* y, void* stream) {
    QA_BEGIN(shape);
    if (!x || !modulus || !y) return SELD_EINVAL;
    p.x = x; p.u = modulus; p.eps = eps; p.o0 = y;
    return qa_pointwise<QA_NORMALIZED>(p, p.M % 4 == 0 && qa_aligned({x, modulus, y}), (hipStream_t)stream);
}

extern "C" int seld_quat_normalized_bwd(const seld_quat_shape* shape, const float* x, const float* modulus, const float* dy,
                                        float eps, float* dx, void* workspace, size_t workspace_bytes, void* stream) {
    QA_BEGIN(shape);
    const int rc = qa_red_check(p);
    if (rc) return rc;
    if (!x || !modulus || !dy || !dx) return SELD_EINVAL;
    const long long floats = qa_red_floats(p);
    if (!workspace || workspace_bytes < (size_t)floats * sizeof(float)) return SELD_EWORKSPACE;
    // G = sum over dim 0 and the components of dy * x, folded into the last row of the workspace
    float* G = (float*)workspace + (floats - (long long)p.S * p.M);
    const bool vec = p.M % 4 == 0 && qa_aligned({x, modulus, dy, dx, workspace});
    p.x = x; p.dy = dy;
    const int r = qa_reduce<true, false>(p, vec, (float*)workspace, G, (hipStream_t)stream);
    if (r) return r;
    p.u = modulus; p.v = G; p.eps = eps; p.o0 = dx;
    return qa_pointwise<QA_NORMALIZED_BWD>(p, vec, (hipStream_t)stream);
}

static int qa_layout(QaP& p, int32_t layout) {
    if (layout != SELD_QUAT_LAYOUT_INPUT && layout != SELD_QUAT_LAYOUT_CAT1) return SELD_EINVAL;
    p.cat1 = layout == SELD_QUAT_LAYOUT_CAT1 && p.S > 1;
    return SELD_OK;
}

template <int OP>
static int qa_unary_fwd(const seld_quat_shape* shape, int32_t layout, const float* x, float* y, void* stream) {
    QA_BEGIN(shape);
    if (qa_layout(p, layout) || !x || !y) return SELD_EINVAL;
    p.x = x; p.o0 = y;
    return qa_pointwise<OP>(p, p.M % 4 == 0 && qa_aligned({x, y}), (hipStream_t)stream);
}

template <int OP>
static int qa_unary_bwd(const seld_quat_shape* shape, int32_t layout, const float* x, const float* dy, float* dx,
                        void* stream) {
    QA_BEGIN(shape);
    if (qa_layout(p, layout) || !x || !dy || !dx) return SELD_EINVAL;
    p.x = x; p.dy = dy; p.o0 = dx;
    return qa_pointwise<OP>(p, p.M % 4 == 0 && qa_aligned({x, dy, dx}), (hipStream_t)stream);
}

extern "C" int seld_quat_normalize_fwd(const seld_quat_shape* shape, int32_t layout, const float* x, float* y, void* stream) {
    return qa_unary_fwd<QA_UNIT>(shape, layout, x, y, stream);
}

extern "C" int seld_quat_normalize_bwd(const seld_quat_shape* shape, int32_t layout, const float* x, const float* dy,
                                       float* dx, void* stream) {
    return qa_unary_bwd<QA_UNIT_BWD>(shape, layout, x, dy, dx, stream);
}

extern "C" int seld_quat_exp_fwd(const seld_quat_shape* shape, int32_t layout, const float* x, float* y, void* stream) {
    return qa_unary_fwd<QA_EXP>(shape, layout, x, y, stream);
}

extern "C" int seld_quat_exp_bwd(const seld_quat_shape* shape, int32_t layout, const float* x, const float* dy, float* dx,
                                 void* stream) {
    return qa_unary_bwd<QA_EXP_BWD>(shape, layout, x, dy, dx, stream);
}

extern "C" int seld_quat_hamilton_fwd(const seld_quat_shape* shape, const float* q0, const float* q1, float* y,
                                      void* stream) {
    QA_BEGIN(shape);
    if (!q0 || !q1 || !y) return SELD_EINVAL;
    p.x = q0; p.x1 = q1; p.o0 = y;
    return qa_pointwise<QA_HPROD>(p, p.M % 4 == 0 && qa_aligned({q0, q1, y}), (hipStream_t)stream);
}

extern "C" int seld_quat_hamilton_bwd(const seld_quat_shape* shape, const float* q0, const float* q1, const float* dy,
                                      float* dq0, float* dq1, void* stream) {
    QA_BEGIN(shape);
    if (!q0 || !q1 || !dy || !dq0 || !dq1) return SELD_EINVAL;
    p.x = q0; p.x1 = q1; p.dy = dy; p.o0 = dq0; p.o1 = dq1;
    return qa_pointwise<QA_HPROD_BWD>(p, p.M % 4 == 0 && qa_aligned({q0, q1, dy, dq0, dq1}), (hipStream_t)stream);
}
