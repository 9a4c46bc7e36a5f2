// Depthwise convolution, gfx950: nn.Conv1d / nn.Conv2d with groups == Cin and Cout = m * Cin (the `depthwise` layer of
// DepthwiseSeparableConv1D / 2D, dual_quaternion_layers.py:19-47 of the reference), exact fp32 on the VALU.
//
//     y[n][o][oh][ow]  = bias[o] + sum_{th, tw} x[n][o / m][oh*sh - ph + th*dh][ow*sw - pw + tw*dw] * w[o][th][tw]
//     dx[n][c][ih][iw] = sum_{j < m} sum_{th, tw : ih = oh*sh - ph + th*dh, iw = ...} dy[n][c*m + j][oh][ow] * w[c*m + j][th][tw]
//     dw[o][th][tw]   += sum_{n, oh, ow} x[n][o / m][...] * dy[n][o][oh][ow],   dbias[o] += sum dy[n][o]
//
// A 3x3 layer does 9 FMAs per 8 bytes moved: every kernel here is bound by HBM, not by arithmetic.  One body serves all
// three (dw_taps): a workgroup owns one plane (n, channel) and a tile of TH x TW results; it stages the window of the
// gathered plane that the tile reads (tile + halo) ONCE in LDS with 16-byte loads along W, then walks the taps in a
// fixed order.  Per axis the result index q and tap t read source index
//     direct map   q*a + b + t*e                         forward (a = stride, b = -pad, e = dil); input gradient at
//                                                        stride 1 (a = 1, b = pad, e = -dil)
//     phase map    (q + pad - t*dil) / s  when s divides it   input gradient with a stride > 1: the quotient and residue
//                                                        of q + pad are formed once per result, those of t*dil advance
//                                                        with the tap, so the test is one compare (no division)
// A thread owns NR rows x NC columns of the tile; its columns are 64 apart (lane + 64*k), so one LDS read instruction
// covers 64 consecutive words (no bank conflict at stride 1) and one store writes 256 contiguous bytes.  The plane's
// weights are wave-uniform (scalar loads), read once per tap.  Windows that do not fit the LDS budget (very large
// dilation x kernel) are read from global memory instead, with the same body.
//
// Weight gradient: each workgroup reduces x * dy over its tile for every tap and for the bias and writes those kh*kw + 1
// partials to the caller's workspace; dwconv_fold_kernel then sums each (channel, tap) over all tiles in a fixed order
// and ADDS into dw / dbias.  No float atomics anywhere: every result is run-to-run bit-identical, with or without
// SELD_DETERMINISTIC.
#include "hc_common.h"

namespace seld {

constexpr int DW_NC = 4;                       // columns per thread
constexpr int DW_LDS_FLOATS = 8192;            // staged window budget: 32 KB
constexpr int DW_BATCH = 8;                    // float4 staging loads in flight per thread

// one axis: extents of the gathered operand / of the result, taps, and the index map (see the file comment)
struct DwAx {
    int src, dst, k;
    int a, b, e;          // direct map
    int s, d, dq, dm;     // phase map: stride, dilation, d / s, d % s
};

struct DwP {
    DwAx h, w;
    int N, Csrc, Cdst, m, KK;
    int WR, WC;           // waves of the workgroup: WR rows x WC columns
    int TH, TW, tiles_w, tiles;
    int rows, pitch;      // staged window (floats: rows * pitch)
    int vec;              // 16-byte staging loads (W % 4 == 0, aligned plane)
    long long src_plane, dst_plane;
    int nsplit;           // weight gradient: partials per (channel, tap) = N * tiles
    const float* src;     // the gathered operand: x (forward, weight gradient) or dy (input gradient)
    const float* wt;      // (Cout, kh*kw)
    const float* bias;
    const float* dy;      // weight gradient
    float* dst;           // y, dx, or the weight-gradient workspace
};

__device__ __forceinline__ int dw_floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// first source index of the window that the results [q0, q0 + T) read
template <bool DIV>
__device__ __forceinline__ int dw_origin(const DwAx& x, int q0) {
    if (DIV) return dw_floor_div(q0 + x.b - (x.k - 1) * x.d, x.s);
    return q0 * x.a + x.b + min(0, (x.k - 1) * x.e);
}

// window rows [r0, r0 + rows) x columns [c0, c0 + pitch) of plane g -> lds, zeros outside the plane
__device__ __forceinline__ void dw_stage(const DwP& p, const float* __restrict__ g, float* lds, int r0, int c0) {
    const int H = p.h.src, W = p.w.src;
    if (p.vec) {                               // c0 and W are multiples of 4: a float4 lies wholly inside or outside
        const int n4 = p.pitch >> 2, tot = p.rows * n4;
        for (int base = 0; base < tot; base += 256 * DW_BATCH) {
            float4 v[DW_BATCH];
#pragma unroll
            for (int u = 0; u < DW_BATCH; ++u) {
                const int it = base + threadIdx.x + 256 * u;
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (it < tot) {
                    const int r = it / n4, gr = r0 + r, gc = c0 + 4 * (it - r * n4);
                    if (gr >= 0 && gr < H && gc >= 0 && gc < W) v[u] = *(const float4*)(g + gr * W + gc);
                }
            }
#pragma unroll
            for (int u = 0; u < DW_BATCH; ++u) {
                const int it = base + threadIdx.x + 256 * u;
                if (it < tot) *(float4*)(lds + 4 * it) = v[u];
            }
        }
    } else {
        const int tot = p.rows * p.pitch;
        for (int base = 0; base < tot; base += 256 * DW_BATCH) {
            float v[DW_BATCH];
#pragma unroll
            for (int u = 0; u < DW_BATCH; ++u) {
                const int it = base + threadIdx.x + 256 * u;
                v[u] = 0.f;
                if (it < tot) {
                    const int r = it / p.pitch, gr = r0 + r, gc = c0 + (it - r * p.pitch);
                    if (gr >= 0 && gr < H && gc >= 0 && gc < W) v[u] = g[gr * W + gc];
                }
            }
#pragma unroll
            for (int u = 0; u < DW_BATCH; ++u) {
                const int it = base + threadIdx.x + 256 * u;
                if (it < tot) lds[it] = v[u];
            }
        }
    }
}

// Walk the taps in order th, tw; for each, f(tap, v) gets the NR x NC source values this thread's results read through
// that tap (0 where the tap does not reach the result or reads padding).  s: the staged window (origin orgh, orgw) or,
// unstaged, the plane itself (origin 0, 0).
template <int NR, int NC, bool DIV, bool STAGED, class F>
__device__ __forceinline__ void dw_taps(const DwP& p, const float* __restrict__ s, int orgh, int orgw, int q0h, int q0w,
                                        F&& f) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wr = wave / p.WC, wc = wave - wr * p.WC;
    int bh[NR], rh[NR], bw[NC], rw[NC];
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int q = q0h + wr + p.WR * i;
        if (DIV) {
            const int num = q + p.h.b, qu = num / p.h.s;
            bh[i] = qu - orgh;
            rh[i] = num - qu * p.h.s;
        } else {
            bh[i] = q * p.h.a + p.h.b - orgh;
            rh[i] = 0;
        }
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int q = q0w + lane + 64 * (wc + p.WC * j);
        if (DIV) {
            const int num = q + p.w.b, qu = num / p.w.s;
            bw[j] = qu - orgw;
            rw[j] = num - qu * p.w.s;
        } else {
            bw[j] = q * p.w.a + p.w.b - orgw;
            rw[j] = 0;
        }
    }
    const int pitch = STAGED ? p.pitch : p.w.src;
    int tdh = 0, tmh = 0;                      // direct: th*e; phase: (th*d) / s, (th*d) % s
    for (int th = 0; th < p.h.k; ++th) {
        int ro[NR];
        bool vh[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            ro[i] = DIV ? bh[i] - tdh : bh[i] + tdh;
            vh[i] = DIV ? rh[i] == tmh : true;
            if (!STAGED) vh[i] = vh[i] && ro[i] >= 0 && ro[i] < p.h.src;
        }
        int tdw = 0, tmw = 0;
        for (int tw = 0; tw < p.w.k; ++tw) {
            int co[NC];
            bool vw[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                co[j] = DIV ? bw[j] - tdw : bw[j] + tdw;
                vw[j] = DIV ? rw[j] == tmw : true;
                if (!STAGED) vw[j] = vw[j] && co[j] >= 0 && co[j] < p.w.src;
            }
            float v[NR][NC];
#pragma unroll
            for (int i = 0; i < NR; ++i)
#pragma unroll
                for (int j = 0; j < NC; ++j) v[i][j] = (vh[i] && vw[j]) ? s[ro[i] * pitch + co[j]] : 0.f;
            f(th * p.w.k + tw, v);
            if (DIV) {
                tdw += p.w.dq;
                tmw += p.w.dm;
                if (tmw >= p.w.s) { tmw -= p.w.s; ++tdw; }
            } else {
                tdw += p.w.e;
            }
        }
        if (DIV) {
            tdh += p.h.dq;
            tmh += p.h.dm;
            if (tmh >= p.h.s) { tmh -= p.h.s; ++tdh; }
        } else {
            tdh += p.h.e;
        }
    }
}

// the tile this workgroup owns: plane (n, channel) and the first result row / column
struct DwTile {
    int n, c, q0h, q0w, tile;
    long long plane;
};

__device__ __forceinline__ DwTile dw_tile(const DwP& p) {
    DwTile t;
    t.plane = blockIdx.x / p.tiles;
    t.tile = blockIdx.x - (int)t.plane * p.tiles;
    t.n = (int)(t.plane / p.Cdst);
    t.c = (int)(t.plane - (long long)t.n * p.Cdst);
    const int ty = t.tile / p.tiles_w;
    t.q0h = ty * p.TH;
    t.q0w = (t.tile - ty * p.tiles_w) * p.TW;
    return t;
}

template <int NR, int NC>
__device__ __forceinline__ void dw_store(const DwP& p, const DwTile& t, const float (&acc)[NR][NC], float b) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wr = wave / p.WC, wc = wave - wr * p.WC;
    float* out = p.dst + t.plane * p.dst_plane;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int qh = t.q0h + wr + p.WR * i;
        if (qh >= p.h.dst) continue;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int qw = t.q0w + lane + 64 * (wc + p.WC * j);
            if (qw < p.w.dst) out[qh * p.w.dst + qw] = acc[i][j] + b;
        }
    }
}

// forward: y = dwconv(x, w) + bias.  Plane (n, o) reads input channel o / m.
template <int NR, bool STAGED>
__global__ __launch_bounds__(256) void dwconv_fwd_kernel(const DwP p) {
    extern __shared__ float lds[];
    const DwTile t = dw_tile(p);
    const float* x = p.src + ((long long)t.n * p.Csrc + t.c / p.m) * p.src_plane;
    int orgh = 0, orgw = 0;
    if (STAGED) {
        orgh = dw_origin<false>(p.h, t.q0h);
        orgw = dw_origin<false>(p.w, t.q0w);
        if (p.vec) orgw &= ~3;
        dw_stage(p, x, lds, orgh, orgw);
        __syncthreads();
    }
    const float* wk = p.wt + (long long)t.c * p.KK;
    float acc[NR][DW_NC] = {};
    dw_taps<NR, DW_NC, false, STAGED>(p, STAGED ? lds : x, orgh, orgw, t.q0h, t.q0w,
                                      [&](int tap, const float (&v)[NR][DW_NC]) {
        const float wv = wk[tap];
#pragma unroll
        for (int i = 0; i < NR; ++i)
#pragma unroll
            for (int j = 0; j < DW_NC; ++j) acc[i][j] = fmaf(v[i][j], wv, acc[i][j]);
    });
    dw_store<NR, DW_NC>(p, t, acc, p.bias ? p.bias[t.c] : 0.f);
}

// input gradient: dx[c] = sum over the m output channels c*m + j of dwconv^T(dy[c*m + j], w[c*m + j])
template <int NR, bool DIV, bool STAGED>
__global__ __launch_bounds__(256) void dwconv_dgrad_kernel(const DwP p) {
    extern __shared__ float lds[];
    const DwTile t = dw_tile(p);
    int orgh = 0, orgw = 0;
    if (STAGED) {
        orgh = dw_origin<DIV>(p.h, t.q0h);
        orgw = dw_origin<DIV>(p.w, t.q0w);
        if (p.vec) orgw &= ~3;
    }
    float acc[NR][DW_NC] = {};
    for (int j = 0; j < p.m; ++j) {
        const int o = t.c * p.m + j;
        const float* dy = p.src + ((long long)t.n * p.Csrc + o) * p.src_plane;
        if (STAGED) {
            if (j) __syncthreads();            // every wave is done with the previous channel's window
            dw_stage(p, dy, lds, orgh, orgw);
            __syncthreads();
        }
        const float* wk = p.wt + (long long)o * p.KK;
        dw_taps<NR, DW_NC, DIV, STAGED>(p, STAGED ? lds : dy, orgh, orgw, t.q0h, t.q0w,
                                        [&](int tap, const float (&v)[NR][DW_NC]) {
            const float wv = wk[tap];
#pragma unroll
            for (int i = 0; i < NR; ++i)
#pragma unroll
                for (int jj = 0; jj < DW_NC; ++jj) acc[i][jj] = fmaf(v[i][jj], wv, acc[i][jj]);
        });
    }
    dw_store<NR, DW_NC>(p, t, acc, 0.f);
}

// weight gradient, first pass: per tile, sum x * dy for every tap and sum dy (the bias); workgroup (plane, tile)
// writes ws[(o * (KK + 1) + tap) * nsplit + n * tiles + tile], tap KK = the bias.  Fixed order throughout.
template <int NR, bool STAGED>
__global__ __launch_bounds__(256) void dwconv_wgrad_kernel(const DwP p) {
    extern __shared__ float lds[];
    const DwTile t = dw_tile(p);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int wr = wave / p.WC, wc = wave - wr * p.WC;
    const float* x = p.src + ((long long)t.n * p.Csrc + t.c / p.m) * p.src_plane;
    const float* dy = p.dy + t.plane * p.dst_plane;
    float g[NR][DW_NC];
    float sb = 0.f;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const int qh = t.q0h + wr + p.WR * i;
#pragma unroll
        for (int j = 0; j < DW_NC; ++j) {
            const int qw = t.q0w + lane + 64 * (wc + p.WC * j);
            g[i][j] = (qh < p.h.dst && qw < p.w.dst) ? dy[qh * p.w.dst + qw] : 0.f;
            sb += g[i][j];
        }
    }
    float* red = lds + (STAGED ? p.rows * p.pitch : 0);      // [KK + 1][4 waves]
    int orgh = 0, orgw = 0;
    if (STAGED) {
        orgh = dw_origin<false>(p.h, t.q0h);
        orgw = dw_origin<false>(p.w, t.q0w);
        if (p.vec) orgw &= ~3;
        dw_stage(p, x, lds, orgh, orgw);
        __syncthreads();
    }
    sb = wave_sum(sb);
    if (lane == 0) red[p.KK * 4 + wave] = sb;
    dw_taps<NR, DW_NC, false, STAGED>(p, STAGED ? lds : x, orgh, orgw, t.q0h, t.q0w,
                                      [&](int tap, const float (&v)[NR][DW_NC]) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NR; ++i)
#pragma unroll
            for (int j = 0; j < DW_NC; ++j) s = fmaf(v[i][j], g[i][j], s);
        s = wave_sum(s);
        if (lane == 0) red[tap * 4 + wave] = s;
    });
    __syncthreads();
    const int split = t.n * p.tiles + t.tile;
    for (int tap = threadIdx.x; tap <= p.KK; tap += 256) {
        const float* r = red + tap * 4;
        p.dst[((long long)t.c * (p.KK + 1) + tap) * p.nsplit + split] = (r[0] + r[1]) + (r[2] + r[3]);
    }
}

// weight gradient, second pass: workgroup (o, tap) sums the nsplit partials in a fixed order and ADDS the sum into
// dw[o][tap] (tap < KK) or dbias[o] (tap == KK)
__global__ __launch_bounds__(256) void dwconv_fold_kernel(const float* __restrict__ ws, int nsplit, int KK, float* dw,
                                                          float* dbias) {
    const int row = blockIdx.x, o = row / (KK + 1), tap = row - o * (KK + 1);
    if (tap == KK && !dbias) return;
    const float* s = ws + (long long)row * nsplit;
    float v = 0.f;
    for (int k = threadIdx.x; k < nsplit; k += 256) v += s[k];
    __shared__ float red[4];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float sum = (red[0] + red[1]) + (red[2] + red[3]);
        if (tap < KK) dw[(long long)o * KK + tap] += sum;
        else dbias[o] += sum;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
enum { DW_FWD = 0, DW_DGRAD = 1, DW_WGRAD = 2 };

struct DwPlan {
    DwP p;
    int nr;
    bool staged, div;
    size_t lds_bytes;
    long long grid;
};

static int dw_validate(const seld_conv_desc* d, int out[2]) {
    if (!d) return SELD_EINVAL;
    if (d->algebra != 1 || (d->ndim != 1 && d->ndim != 2)) return SELD_EINVAL;
    if (d->N <= 0 || d->Cin <= 0 || d->Cout <= 0) return SELD_EINVAL;
    if (d->groups != d->Cin || d->Cout % d->Cin) return SELD_EINVAL;
    for (int i = 0; i < 2; ++i)
        if (d->in[i] <= 0 || d->k[i] <= 0 || d->stride[i] <= 0 || d->dil[i] <= 0 || d->pad[i] < 0) return SELD_EINVAL;
    if (d->ndim == 1 && (d->in[0] != 1 || d->k[0] != 1 || d->pad[0] != 0)) return SELD_EINVAL;
    for (int i = 0; i < 2; ++i) {
        const long long span = (long long)d->dil[i] * (d->k[i] - 1) + 1, padded = (long long)d->in[i] + 2LL * d->pad[i];
        if (padded < span) return SELD_EINVAL;                        // empty output
        if (padded >= (1LL << 28) || span >= (1LL << 28)) return SELD_EUNSUPPORTED;
        out[i] = (int)((padded - span) / d->stride[i] + 1);
    }
    if (d->k[0] * d->k[1] > 255) return SELD_EUNSUPPORTED;
    // one image of either operand is indexed with 32-bit offsets
    if ((long long)d->Cin * d->in[0] * d->in[1] >= (1LL << 28)) return SELD_EUNSUPPORTED;
    if ((long long)d->Cout * out[0] * out[1] >= (1LL << 28)) return SELD_EUNSUPPORTED;
    return SELD_OK;
}

// window extent along one axis for T results
static long long dw_extent(const DwAx& x, int T, bool div) {
    if (div) return (T - 1 + (long long)(x.k - 1) * x.d) / x.s + 2;
    return (long long)(T - 1) * x.a + (long long)(x.k - 1) * (x.e < 0 ? -x.e : x.e) + 1;
}

// The tile and the window depend on the descriptor alone (the workspace size must not depend on pointers); `src`
// only decides whether the window is staged with 16-byte loads.
static int dw_plan(const seld_conv_desc* d, int which, const void* src, DwPlan* pl) {
    int o[2];
    const int rc = dw_validate(d, o);
    if (rc) return rc;
    DwPlan q{};
    DwP& p = q.p;
    const bool dg = which == DW_DGRAD;
    DwAx* ax[2] = {&p.h, &p.w};
    for (int i = 0; i < 2; ++i) {
        DwAx& a = *ax[i];
        a.k = d->k[i];
        a.s = d->stride[i];
        a.d = d->dil[i];
        a.dq = a.d / a.s;
        a.dm = a.d % a.s;
        if (dg) {
            a.src = o[i]; a.dst = d->in[i];
            a.a = 1; a.b = d->pad[i]; a.e = -d->dil[i];
        } else {
            a.src = d->in[i]; a.dst = o[i];
            a.a = d->stride[i]; a.b = -d->pad[i]; a.e = d->dil[i];
        }
    }
    q.div = dg && (d->stride[0] > 1 || d->stride[1] > 1);
    p.N = d->N;
    p.m = d->Cout / d->Cin;
    p.Csrc = dg ? d->Cout : d->Cin;
    p.Cdst = dg ? d->Cin : d->Cout;
    p.KK = d->k[0] * d->k[1];
    p.src_plane = (long long)p.h.src * p.w.src;
    p.dst_plane = (long long)p.h.dst * p.w.dst;
    p.vec = p.w.src % 4 == 0 && ((uintptr_t)src & 15) == 0;
    // tile: NR rows x 4 columns per thread, 64 lanes x WC waves across, WR = 4 / WC waves down
    const int dh = p.h.dst, dwd = p.w.dst;
    const int wc_w = dwd > 512 ? 4 : dwd > 256 ? 2 : 1;
    const int wc_1 = dh >= 4 ? wc_w : dh >= 2 ? (wc_w > 2 ? wc_w : 2) : 4;
    const int cand[3][2] = {{dh >= 8 ? 4 : 1, dh >= 8 ? wc_w : wc_1}, {1, wc_1}, {1, 1}};
    int pick = -1;
    for (int c = 0; c < 3 && pick < 0; ++c) {
        const int WR = 4 / cand[c][1];
        const long long rows = dw_extent(p.h, WR * cand[c][0], q.div);
        const long long pitch = (dw_extent(p.w, 64 * cand[c][1] * DW_NC, q.div) + 3 + 3) & ~3LL;  // + origin alignment
        if (rows * pitch <= DW_LDS_FLOATS) {
            pick = c;
            p.rows = (int)rows;
            p.pitch = (int)pitch;
        }
    }
    q.staged = pick >= 0;
    if (pick < 0) pick = 0;
    q.nr = cand[pick][0];
    p.WC = cand[pick][1];
    p.WR = 4 / p.WC;
    p.TH = p.WR * q.nr;
    p.TW = 64 * p.WC * DW_NC;
    p.tiles_w = (dwd + p.TW - 1) / p.TW;
    const long long tiles = (long long)((dh + p.TH - 1) / p.TH) * p.tiles_w;
    q.grid = (long long)p.N * p.Cdst * tiles;
    if (q.grid >= (1LL << 31)) return SELD_EUNSUPPORTED;
    p.tiles = (int)tiles;
    p.nsplit = (int)(p.N * tiles);
    if (!q.staged) p.rows = p.pitch = 0;
    q.lds_bytes = (size_t)p.rows * p.pitch * sizeof(float) + (which == DW_WGRAD ? 16 * (p.KK + 1) : 0);
    if (which == DW_WGRAD && (long long)d->Cout * (p.KK + 1) >= (1LL << 31)) return SELD_EUNSUPPORTED;
    *pl = q;
    return SELD_OK;
}

static size_t dw_wgrad_bytes(const DwPlan& q) { return (size_t)q.p.Cdst * (q.p.KK + 1) * q.p.nsplit * sizeof(float); }

static void dw_label(const DwPlan& q, int which, char* buf, int buflen) {
    const int st = q.staged ? 1 : 0;
    if (which == DW_FWD) snprintf(buf, buflen, "dwconv_fwd_kernel<%d, %s>", q.nr, st ? "true" : "false");
    else if (which == DW_DGRAD)
        snprintf(buf, buflen, "dwconv_dgrad_kernel<%d, %s, %s>", q.nr, q.div ? "true" : "false", st ? "true" : "false");
    else snprintf(buf, buflen, "dwconv_wgrad_kernel<%d, %s>", q.nr, st ? "true" : "false");
}

template <int NR, bool ST>
static void dw_launch(const DwPlan& q, int which, hipStream_t st) {
    const dim3 grid((unsigned)q.grid), blk(256);
    if (which == DW_FWD) hipLaunchKernelGGL((dwconv_fwd_kernel<NR, ST>), grid, blk, q.lds_bytes, st, q.p);
    else if (which == DW_WGRAD) hipLaunchKernelGGL((dwconv_wgrad_kernel<NR, ST>), grid, blk, q.lds_bytes, st, q.p);
    else if (q.div) hipLaunchKernelGGL((dwconv_dgrad_kernel<NR, true, ST>), grid, blk, q.lds_bytes, st, q.p);
    else hipLaunchKernelGGL((dwconv_dgrad_kernel<NR, false, ST>), grid, blk, q.lds_bytes, st, q.p);
}

static int dw_run(const DwPlan& q, int which, hipStream_t st) {
    if (q.nr == 4) {
        if (q.staged) dw_launch<4, true>(q, which, st);
        else dw_launch<4, false>(q, which, st);
    } else {
        if (q.staged) dw_launch<1, true>(q, which, st);
        else dw_launch<1, false>(q, which, st);
    }
    return check_launch();
}

}  // namespace seld

using namespace seld;

extern "C" int seld_dwconv_out_shape(const seld_conv_desc* d, int32_t out[2]) {
    int o[2];
    const int rc = dw_validate(d, o);
    if (rc) return rc;
    if (out) out[0] = o[0], out[1] = o[1];
    return SELD_OK;
}

extern "C" int seld_dwconv_fwd(const seld_conv_desc* d, const float* x, const float* w, const float* bias, float* y,
                               void* stream) {
    DwPlan q;
    const int rc = dw_plan(d, DW_FWD, x, &q);
    if (rc) return rc;
    if (!x || !w || !y) return SELD_EINVAL;
    q.p.src = x; q.p.wt = w; q.p.bias = bias; q.p.dst = y;
    return dw_run(q, DW_FWD, (hipStream_t)stream);
}

extern "C" int seld_dwconv_bwd_data(const seld_conv_desc* d, const float* dy, const float* w, float* dx, void* stream) {
    DwPlan q;
    const int rc = dw_plan(d, DW_DGRAD, dy, &q);
    if (rc) return rc;
    if (!dy || !w || !dx) return SELD_EINVAL;
    q.p.src = dy; q.p.wt = w; q.p.dst = dx;
    return dw_run(q, DW_DGRAD, (hipStream_t)stream);
}

extern "C" size_t seld_dwconv_bwd_weight_workspace(const seld_conv_desc* d) {
    DwPlan q;
    if (dw_plan(d, DW_WGRAD, nullptr, &q) != SELD_OK) return 0;
    return dw_wgrad_bytes(q);
}

extern "C" int seld_dwconv_bwd_weight_acc(const seld_conv_desc* d, const float* x, const float* dy, float* dw,
                                          float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
    DwPlan q;
    const int rc = dw_plan(d, DW_WGRAD, x, &q);
    if (rc) return rc;
    if (!x || !dy || !dw) return SELD_EINVAL;
    if (!workspace || workspace_bytes < dw_wgrad_bytes(q)) return SELD_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    q.p.src = x; q.p.dy = dy; q.p.dst = (float*)workspace;
    int r = dw_run(q, DW_WGRAD, st);
    if (r) return r;
    hipLaunchKernelGGL(dwconv_fold_kernel, dim3((unsigned)(q.p.Cdst * (q.p.KK + 1))), dim3(256), 0, st,
                       (const float*)workspace, q.p.nsplit, q.p.KK, dw, dbias);
    return check_launch();
}

extern "C" int seld_dwconv_kernel_label(const seld_conv_desc* d, int32_t which, char* buf, int32_t buflen) {
    if (which < 0 || which > 2) return SELD_EINVAL;
    DwPlan q;
    const int rc = dw_plan(d, which, nullptr, &q);
    if (rc) return rc;
    if (!buf || buflen < 48) return SELD_EINVAL;
    dw_label(q, which, buf, buflen);
    return SELD_OK;
}
