// Hypercomplex (real / quaternion / dual-quaternion) 3-D convolution and transposed convolution, gfx950
// (F.conv3d / F.conv_transpose3d of quaternion_ops.py:125-171 and dual_quaternion_ops.py:111-153 of the reference).
//
//     conv            y[n][co][o]  = bias[co] + sum_{ci, t} x[n][ci][o*s - p + t*d] * M[co][ci][t]
//     transposed conv y[n][co][o]  = bias[co] + sum_{ci, t : o = i*s - p + t*d} u[n][ci][i] * M[ci][co][t]
//
// per axis (D, H, W); M is the Hamilton block matrix of the component tensors, read directly with the signs applied
// while staging into LDS (hc_comp), never materialised.  Three kernels serve both operations:
//
//   hc_conv3d_fwd_kernel    the implicit GEMM of hc_phase_gemm.h on three axes with its forward map: positions
//                           (n, od, oh, ow) x reduction (ci, td, th, tw).  Conv forward (+ bias), transposed-conv input
//                           gradient
//   hc_conv3d_phase_kernel  the same body with its stride-phase map and the weights read transposed: sd*sh*sw residue
//                           classes, a dense stride-1 GEMM per class.  Transposed-conv forward (+ bias; positions no tap
//                           reaches get the bias alone), conv input gradient
//   hc_conv3d_wgrad_kernel  G = sum dy (x) im2col(x), split over positions into a workspace of partials;
//                           hc_conv3d_fold_kernel then sums the splits in a fixed order, folds the block matrix onto the
//                           components and ADDS into dw[c] (and the bias partials into dbias)
//
// The GEMM body, its index maps, the dual quaternion's zero-quadrant skip, the tile choice and the launch are described
// and live in hc_phase_gemm.h; this file keeps the 3-D descriptor checks, the weight gradient and the entry points.
//
// No float atomics anywhere: every result is run-to-run bit-identical, with or without SELD_DETERMINISTIC.
#include "hc_phase_gemm.h"

namespace seld {

typedef PgP<3> C3P;

template <int CT, int PT>
__global__ __launch_bounds__(256) void hc_conv3d_fwd_kernel(const C3P p) { pg_gemm<CT, PT, false, 3>(p); }

template <int CT, int PT>
__global__ __launch_bounds__(256) void hc_conv3d_phase_kernel(const C3P p) { pg_gemm<CT, PT, true, 3>(p); }

// ------------------------------------------------------------------------------------------
// weight gradient: G[co][c] = sum_pos dy[n][co][pos] * x[n][ci][pos*s - p + tap*d], c = ci*KK + tap
// ------------------------------------------------------------------------------------------
struct C3W {
    int A, N, Ci, Co;              // channels of x (columns Ci*KK) / of dy (rows)
    int in[3], out[3], k[3], s[3], pad[3], dil[3];
    int KK, Kc;                    // Kc = Ci*KK
    int ntn;                       // column tiles
    long long So, Si;
    long long Ptot;                // N*So
    long long split_len;           // positions per split (multiple of 16)
    int nsplit;
    const float* x;
    const float* dy;
    float* ws;                     // [nsplit][Co][Kc] partials
};

// 64 x 64 tile of G per workgroup over one split of the positions; 4 waves of 32 x 32 (2 x 2 MFMA tiles).  Thread
// (row = tid/4, g = tid%4) stages positions 4g..4g+3 of each 16-position chunk: dy row `row` and im2col column `row`.
__global__ __launch_bounds__(256) void hc_conv3d_wgrad_kernel(const C3W p) {
    __shared__ __attribute__((aligned(16))) float As[2][4][64][4];
    __shared__ __attribute__((aligned(16))) float Bs[2][4][64][4];

    const int split = blockIdx.x;
    const int mt = blockIdx.y / p.ntn, nt = blockIdx.y - (blockIdx.y / p.ntn) * p.ntn;
    const int m0 = mt * 64, n0 = nt * 64;
    // dual quaternion: a tile wholly in the zero quadrant (low dy rows x high x channels) is never read by the fold
    if (p.A == 8 && m0 + 64 <= (p.Co >> 1) && n0 >= (p.Ci >> 1) * p.KK) return;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int row = tid >> 2, g = tid & 3;

    const long long pbeg = (long long)split * p.split_len;
    const long long pend = min(pbeg + p.split_len, p.Ptot);
    const int nchunks = (int)((pend - pbeg + 15) >> 4);

    // this thread's dy row and im2col column
    const int co = m0 + row;
    const bool co_ok = co < p.Co;
    const int c = n0 + row;
    const bool c_ok = c < p.Kc;
    const int cc = c_ok ? c : 0;
    const int ci = cc / p.KK;
    int tap = cc - ci * p.KK;
    const int kd = tap / (p.k[1] * p.k[2]);
    tap -= kd * p.k[1] * p.k[2];
    const int kh = tap / p.k[2], kw = tap - (tap / p.k[2]) * p.k[2];
    const int offd = kd * p.dil[0] - p.pad[0], offh = kh * p.dil[1] - p.pad[1], offw = kw * p.dil[2] - p.pad[2];

    // position cursor of this thread's first staged position of the next chunk
    long long cn;
    int cd, ch, cw;
    {
        const long long q = pbeg + 4 * g;
        cn = q / p.So;
        int rem = (int)(q - cn * p.So);
        cd = rem / (p.out[1] * p.out[2]);
        rem -= cd * p.out[1] * p.out[2];
        ch = rem / p.out[2];
        cw = rem - ch * p.out[2];
    }
    auto advance = [&](int k, long long& n, int& d, int& h, int& w) __attribute__((always_inline)) {
        w += k;
        while (w >= p.out[2]) {
            w -= p.out[2];
            if (++h == p.out[1]) {
                h = 0;
                if (++d == p.out[0]) { d = 0; ++n; }
            }
        }
    };
    long long cpos = pbeg + 4 * g;

    float ar[4], br[4];
    auto load_chunk = [&]() __attribute__((always_inline)) {
        long long n = cn;
        int d = cd, h = ch, w = cw;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool pv = cpos + e < pend;
            const long long sp = ((long long)d * p.out[1] + h) * p.out[2] + w;
            ar[e] = (pv && co_ok) ? p.dy[(n * p.Co + co) * p.So + sp] : 0.f;
            const int id = d * p.s[0] + offd, ih = h * p.s[1] + offh, iw = w * p.s[2] + offw;
            const bool xin = pv && c_ok && (unsigned)id < (unsigned)p.in[0] && (unsigned)ih < (unsigned)p.in[1] &&
                             (unsigned)iw < (unsigned)p.in[2];
            br[e] = xin ? p.x[(n * p.Ci + ci) * p.Si + ((long long)id * p.in[1] + ih) * p.in[2] + iw] : 0.f;
            if (e < 3) advance(1, n, d, h, w);
        }
        advance(16, cn, cd, ch, cw);
        cpos += 16;
    };
    auto store_chunk = [&](int buf) __attribute__((always_inline)) {
        *reinterpret_cast<float4*>(&As[buf][g][row][0]) = make_float4(ar[0], ar[1], ar[2], ar[3]);
        *reinterpret_cast<float4*>(&Bs[buf][g][row][0]) = make_float4(br[0], br[1], br[2], br[3]);
    };

    floatx4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (floatx4){0.f, 0.f, 0.f, 0.f};
    const int fr = lane & 15, fk = lane >> 4;
    const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;

    if (nchunks > 0) {
        load_chunk();
        store_chunk(0);
    }
    __syncthreads();
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        const int buf = chunk & 1;
        if (chunk + 1 < nchunks) load_chunk();
        float av[2][4], bv[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float4 t = *reinterpret_cast<const float4*>(&As[buf][fk][wm0 + i * 16 + fr][0]);
            av[i][0] = t.x; av[i][1] = t.y; av[i][2] = t.z; av[i][3] = t.w;
            const float4 u = *reinterpret_cast<const float4*>(&Bs[buf][fk][wn0 + i * 16 + fr][0]);
            bv[i][0] = u.x; bv[i][1] = u.y; bv[i][2] = u.z; bv[i][3] = u.w;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][s], bv[j][s], acc[i][j], 0, 0, 0);
        if (chunk + 1 < nchunks) store_chunk(buf ^ 1);
        __syncthreads();
    }

    // lane holds G rows 4 fk + r, column fr of each 16 x 16 tile
    float* out = p.ws + (size_t)split * p.Co * p.Kc;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int cj = n0 + wn0 + j * 16 + fr;
            if (cj >= p.Kc) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ri = m0 + wm0 + i * 16 + fk * 4 + r;
                if (ri < p.Co) out[(size_t)ri * p.Kc + cj] = acc[i][j][r];
            }
        }
}

// Partial channel sums of t (N, C, S) over position block blockIdx.y of blen positions: bws[b][c]; fixed order.
__global__ __launch_bounds__(256) void hc_conv3d_bias_kernel(const float* __restrict__ t, int N, int C, long long S,
                                                             long long blen, float* __restrict__ bws) {
    const int c = blockIdx.x, b = blockIdx.y;
    const long long beg = (long long)b * blen;
    const long long end = min(beg + blen, (long long)N * S);
    float s = 0.f;
    for (long long q = beg + threadIdx.x; q < end; q += 256) {
        const long long n = q / S;
        s += t[(n * C + c) * S + (q - n * S)];
    }
    __shared__ float red[4];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) bws[(size_t)b * C + c] = red[0] + red[1] + red[2] + red[3];
}

// dw[c][o][i][tap] += sum over the blocks (P, Q) of component c of sign * sum_split G[P*OA + o][(Q*IA + i)*KK + tap];
// threads past the weights: dbias[c] += sum_b bws[b][c], c < nbc.  Fixed order throughout.
__global__ __launch_bounds__(256) void hc_conv3d_fold_kernel(const float* __restrict__ ws, int nsplit, int A, int Co,
                                                             int Ci, int KK, WPtrsMut dw, const float* __restrict__ bws,
                                                             int nbias, int nbc, float* dbias) {
    const int OA = Co / A, IA = Ci / A;
    const long long per = (long long)OA * IA * KK;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long Kc = (long long)Ci * KK;
    if (e < A * per) {
        const int comp = (int)(e / per);
        const long long r = e - comp * per;
        const int o = (int)(r / ((long long)IA * KK));
        const int it = (int)(r - (long long)o * IA * KK);       // i*KK + tap
        float sum = 0.f;
        for (int P = 0; P < A; ++P)
            for (int Q = 0; Q < A; ++Q) {
                bool zero, neg;
                if (hc_comp(A, P, Q, &zero, &neg) != comp || zero) continue;
                const float* src = ws + (long long)(P * OA + o) * Kc + (long long)Q * IA * KK + it;
                float s = 0.f;
                for (int k = 0; k < nsplit; ++k) s += src[(long long)k * Co * Kc];
                sum += neg ? -s : s;
            }
        dw.p[comp][r] += sum;
    } else if (dbias && e - A * per < nbc) {
        const int co = (int)(e - A * per);
        float s = 0.f;
        for (int b = 0; b < nbias; ++b) s += bws[(size_t)b * nbc + co];
        dbias[co] += s;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static long long vol3(const int v[3]) { return (long long)v[0] * v[1] * v[2]; }

// descriptor checks shared by the convolution and the transposed convolution
static int c3_validate(const seld_conv3d_desc* d) {
    if (!d) return SELD_EINVAL;
    if (d->algebra != 1 && d->algebra != 4 && d->algebra != 8) return SELD_EINVAL;
    if (d->groups != 1) return SELD_EUNSUPPORTED;
    if (d->N <= 0 || d->Cin <= 0 || d->Cout <= 0) return SELD_EINVAL;
    if (d->Cin % d->algebra || d->Cout % d->algebra) return SELD_EINVAL;
    for (int i = 0; i < 3; ++i)
        if (d->in[i] <= 0 || d->k[i] <= 0 || d->stride[i] <= 0 || d->dil[i] <= 0 || d->pad[i] < 0) return SELD_EINVAL;
    for (int i = 0; i < 3; ++i)
        if (d->stride[i] > PG_MAXS) return SELD_EUNSUPPORTED;          // phase tables
    const long long KK = vol3(d->k);
    if (KK > 4096) return SELD_EUNSUPPORTED;
    // component tensors and one image of either operand are addressed with 32-bit offsets
    if ((long long)(d->Cout / d->algebra) * (d->Cin / d->algebra) * KK >= (1LL << 31)) return SELD_EUNSUPPORTED;
    if ((long long)d->Cout * d->Cin * KK >= (1LL << 29)) return SELD_EUNSUPPORTED;   // weight-gradient partials
    if ((long long)d->Cin * vol3(d->in) >= (1LL << 28)) return SELD_EUNSUPPORTED;
    return SELD_OK;
}

static int c3_conv_out(const seld_conv3d_desc* d, int out[3]) {
    int rc = c3_validate(d);
    if (rc) return rc;
    for (int i = 0; i < 3; ++i) {
        const int num = d->in[i] + 2 * d->pad[i] - d->dil[i] * (d->k[i] - 1) - 1;
        if (num < 0) return SELD_EINVAL;
        out[i] = num / d->stride[i] + 1;
    }
    if ((long long)d->Cout * vol3(out) >= (1LL << 28)) return SELD_EUNSUPPORTED;
    return SELD_OK;
}

// transposed: per axis (in - 1)*s - 2p + d*(k - 1) + op + 1, PyTorch's rule op < s or op < d; algebra 1 and 4
static int c3_tconv_out(const seld_conv3d_desc* d, const int32_t op[3], int out[3]) {
    int rc = c3_validate(d);
    if (rc) return rc;
    if (!op) return SELD_EINVAL;
    for (int i = 0; i < 3; ++i) {
        if (op[i] < 0 || (op[i] >= d->stride[i] && op[i] >= d->dil[i])) return SELD_EINVAL;
        out[i] = (d->in[i] - 1) * d->stride[i] - 2 * d->pad[i] + d->dil[i] * (d->k[i] - 1) + op[i] + 1;
        if (out[i] <= 0) return SELD_EINVAL;
    }
    if (d->algebra == 8) return SELD_EUNSUPPORTED;     // the reference has no dual-quaternion transposed convolution
    if ((long long)d->Cout * vol3(out) >= (1LL << 28)) return SELD_EUNSUPPORTED;
    return SELD_OK;
}

// geometry of one GEMM / weight-gradient launch in convolution terms: x (Ci, in) -> y (Co, out)
typedef PgGeom<3> G3;

static G3 g3_of(const seld_conv3d_desc* d, const int out[3], bool mirror) {
    G3 g;
    g.A = d->algebra; g.N = d->N;
    g.Ci = mirror ? d->Cout : d->Cin;
    g.Co = mirror ? d->Cin : d->Cout;
    for (int i = 0; i < 3; ++i) {
        g.in[i] = mirror ? out[i] : d->in[i];
        g.out[i] = mirror ? d->in[i] : out[i];
        g.k[i] = d->k[i]; g.s[i] = d->stride[i]; g.p[i] = d->pad[i]; g.d[i] = d->dil[i];
    }
    return g;
}

// the kernel of tile c: the five tiles of the 3-D tile choice, forward or phase map
static auto c3_kernel(PgCfg c, bool phase) -> void (*)(const C3P) {
    if (c.ct == 12) return phase ? hc_conv3d_phase_kernel<12, 1> : hc_conv3d_fwd_kernel<12, 1>;
    if (c.ct == 4 && c.pt == 1) return phase ? hc_conv3d_phase_kernel<4, 1> : hc_conv3d_fwd_kernel<4, 1>;
    if (c.ct == 2) return phase ? hc_conv3d_phase_kernel<2, 4> : hc_conv3d_fwd_kernel<2, 4>;
    if (c.ct == 1) return phase ? hc_conv3d_phase_kernel<1, 4> : hc_conv3d_fwd_kernel<1, 4>;
    return phase ? hc_conv3d_phase_kernel<4, 4> : hc_conv3d_fwd_kernel<4, 4>;
}

// one GEMM launch: every check before the launch, nothing written on refusal
static int c3_gemm_run(const G3& g, bool phase, const float* x, const float* const w[8], const float* bias, float* y,
                       hipStream_t st, char* label, int buflen) {
    C3P p{};
    pg_fill(p, g, phase, w);
    int rc = pg_addressable(p);
    if (rc) return rc;
    const PgCfg c = pg_cfg(p, true);
    if (label) {
        snprintf(label, buflen, "%s<%d, %d>", phase ? "hc_conv3d_phase_kernel" : "hc_conv3d_fwd_kernel", c.ct, c.pt);
        return SELD_OK;
    }
    if (!x || !w || !y) return SELD_EINVAL;
    p.x = x; p.bias = bias; p.y = y;
    return pg_launch(c3_kernel(c, phase), c, p, st);
}

// weight-gradient plan: position splits so that the grid fills the GPU, bias blocks likewise; workspace floats
struct C3Plan {
    C3W w;
    int ntm, nbias;
    long long blen;
    size_t ws_floats, bias_floats;
};

static C3Plan c3_plan(const G3& g) {
    C3Plan pl{};
    C3W& w = pl.w;
    w.A = g.A; w.N = g.N; w.Ci = g.Ci; w.Co = g.Co;
    for (int i = 0; i < 3; ++i) {
        w.in[i] = g.in[i]; w.out[i] = g.out[i]; w.k[i] = g.k[i];
        w.s[i] = g.s[i]; w.pad[i] = g.p[i]; w.dil[i] = g.d[i];
    }
    w.KK = g.k[0] * g.k[1] * g.k[2];
    w.Kc = g.Ci * w.KK;
    w.So = vol3(g.out); w.Si = vol3(g.in);
    w.Ptot = (long long)g.N * w.So;
    w.ntn = (w.Kc + 63) / 64;
    pl.ntm = (g.Co + 63) / 64;
    const long long tiles = (long long)pl.ntm * w.ntn;
    long long ns = (1024 + tiles - 1) / tiles;                       // about 4 workgroups per CU
    const long long by_len = (w.Ptot + 255) / 256;                   // at least 16 chunks per split
    const long long by_mem = (1LL << 26) / ((long long)g.Co * w.Kc); // partials <= 256 MB
    if (ns > by_len) ns = by_len;
    if (ns > by_mem) ns = by_mem;
    if (ns < 1) ns = 1;
    w.split_len = ((w.Ptot + ns - 1) / ns + 15) / 16 * 16;
    w.nsplit = (int)((w.Ptot + w.split_len - 1) / w.split_len);
    pl.ws_floats = (size_t)w.nsplit * g.Co * w.Kc;
    // bias: the channel sums of dy (conv) / x (the mirrored convolution of the transposed one) -- rows of the caller
    pl.nbias = 1;
    pl.blen = 1;
    pl.bias_floats = 0;
    return pl;
}

static void c3_bias_plan(C3Plan& pl, int C, long long total) {
    long long nb = (2048 + C - 1) / C;
    const long long by_len = (total + 4095) / 4096;
    if (nb > by_len) nb = by_len;
    if (nb < 1) nb = 1;
    pl.blen = (total + nb - 1) / nb;
    pl.nbias = (int)((total + pl.blen - 1) / pl.blen);
    pl.bias_floats = (size_t)pl.nbias * C;
}

// bias_t: the tensor (N, bias_C, bias_S) whose channel sums are the bias gradient
static size_t c3_wgrad_bytes(const G3& g, int bias_C, long long bias_S) {
    C3Plan pl = c3_plan(g);
    c3_bias_plan(pl, bias_C, (long long)g.N * bias_S);
    return (pl.ws_floats + pl.bias_floats) * sizeof(float);
}

static int c3_wgrad_run(const G3& g, const float* x, const float* dy, float* const dw[8], float* dbias,
                        const float* bias_t, int bias_C, long long bias_S, void* workspace, size_t workspace_bytes,
                        hipStream_t st) {
    if (!x || !dy || !dw) return SELD_EINVAL;
    for (int i = 0; i < g.A; ++i)
        if (!dw[i]) return SELD_EINVAL;
    C3Plan pl = c3_plan(g);
    c3_bias_plan(pl, bias_C, (long long)g.N * bias_S);
    if (!workspace || workspace_bytes < (pl.ws_floats + pl.bias_floats) * sizeof(float)) return SELD_EWORKSPACE;
    const long long ngrid = (long long)pl.ntm * pl.w.ntn;
    if (ngrid >= 65536) return SELD_EUNSUPPORTED;
    float* ws = (float*)workspace;
    float* bws = ws + pl.ws_floats;
    pl.w.x = x; pl.w.dy = dy; pl.w.ws = ws;
    hipLaunchKernelGGL(hc_conv3d_wgrad_kernel, dim3(pl.w.nsplit, (unsigned)ngrid), dim3(256), 0, st, pl.w);
    int rc = check_launch();
    if (rc) return rc;
    if (dbias) {
        hipLaunchKernelGGL(hc_conv3d_bias_kernel, dim3(bias_C, pl.nbias), dim3(256), 0, st, bias_t, g.N, bias_C, bias_S,
                           pl.blen, bws);
        rc = check_launch();
        if (rc) return rc;
    }
    WPtrsMut d{};
    for (int i = 0; i < 8; ++i) d.p[i] = i < g.A ? dw[i] : nullptr;
    const long long nw = (long long)g.Co * g.Ci / g.A * pl.w.KK + (dbias ? bias_C : 0);
    hipLaunchKernelGGL(hc_conv3d_fold_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, ws, pl.w.nsplit,
                       g.A, g.Co, g.Ci, pl.w.KK, d, bws, pl.nbias, bias_C, dbias);
    return check_launch();
}

}  // namespace seld

using namespace seld;

// ---- convolution ----------------------------------------------------------------------------------------------------
extern "C" int seld_hc_conv3d_out_shape(const seld_conv3d_desc* d, int32_t out[3]) {
    int o[3];
    const int rc = c3_conv_out(d, o);
    if (rc) return rc;
    if (out) for (int i = 0; i < 3; ++i) out[i] = o[i];
    return SELD_OK;
}

extern "C" int seld_hc_conv3d_fwd(const seld_conv3d_desc* d, const float* x, const float* const w[8], const float* bias,
                                  float* y, void* stream) {
    int o[3];
    const int rc = c3_conv_out(d, o);
    if (rc) return rc;
    return c3_gemm_run(g3_of(d, o, false), false, x, w, bias, y, (hipStream_t)stream, nullptr, 0);
}

// dx = conv_transpose(dy, M) on the phase kernel, cut to the input extent
extern "C" int seld_hc_conv3d_bwd_data(const seld_conv3d_desc* d, const float* dy, const float* const w[8], float* dx,
                                       void* stream) {
    int o[3];
    const int rc = c3_conv_out(d, o);
    if (rc) return rc;
    return c3_gemm_run(g3_of(d, o, true), true, dy, w, nullptr, dx, (hipStream_t)stream, nullptr, 0);
}

extern "C" size_t seld_hc_conv3d_bwd_weight_workspace(const seld_conv3d_desc* d) {
    int o[3];
    if (c3_conv_out(d, o) != SELD_OK) return 0;
    return c3_wgrad_bytes(g3_of(d, o, false), d->Cout, vol3(o));
}

// dw[c] += weight gradient, dbias (nullable) += channel sums of dy
extern "C" int seld_hc_conv3d_bwd_weight_acc(const seld_conv3d_desc* d, const float* x, const float* dy,
                                             float* const dw[8], float* dbias, void* workspace, size_t workspace_bytes,
                                             void* stream) {
    int o[3];
    const int rc = c3_conv_out(d, o);
    if (rc) return rc;
    return c3_wgrad_run(g3_of(d, o, false), x, dy, dw, dbias, dy, d->Cout, vol3(o), workspace, workspace_bytes,
                        (hipStream_t)stream);
}

extern "C" int seld_hc_conv3d_kernel_label(const seld_conv3d_desc* d, int32_t which, char* buf, int32_t buflen) {
    int o[3];
    const int rc = c3_conv_out(d, o);
    if (rc) return rc;
    if (!buf || buflen < 48 || which < 0 || which > 2) return SELD_EINVAL;
    if (which == 2) {
        snprintf(buf, buflen, "hc_conv3d_wgrad_kernel");
        return SELD_OK;
    }
    return c3_gemm_run(g3_of(d, o, which == 1), which == 1, nullptr, nullptr, nullptr, nullptr, nullptr, buf, buflen);
}

// ---- transposed convolution (d: Cin / in = the transposed convolution's input) ------------------------------------
extern "C" int seld_hc_conv3d_transpose_out_shape(const seld_conv3d_desc* d, const int32_t out_pad[3], int32_t out[3]) {
    int o[3];
    const int rc = c3_tconv_out(d, out_pad, o);
    if (rc) return rc;
    if (out) for (int i = 0; i < 3; ++i) out[i] = o[i];
    return SELD_OK;
}

// y = conv_transpose(x, M) + bias on the phase kernel: the convolution (Cin, in) -> (Cout, out) with transposed weights
extern "C" int seld_hc_conv3d_transpose_fwd(const seld_conv3d_desc* d, const int32_t out_pad[3], const float* x,
                                            const float* const w[8], const float* bias, float* y, void* stream) {
    int o[3];
    const int rc = c3_tconv_out(d, out_pad, o);
    if (rc) return rc;
    return c3_gemm_run(g3_of(d, o, false), true, x, w, bias, y, (hipStream_t)stream, nullptr, 0);
}

// dx = conv(dy, M) with the same stride / padding / dilation on the forward kernel, cut to the input extent
extern "C" int seld_hc_conv3d_transpose_bwd_data(const seld_conv3d_desc* d, const int32_t out_pad[3], const float* dy,
                                                 const float* const w[8], float* dx, void* stream) {
    int o[3];
    const int rc = c3_tconv_out(d, out_pad, o);
    if (rc) return rc;
    return c3_gemm_run(g3_of(d, o, true), false, dy, w, nullptr, dx, (hipStream_t)stream, nullptr, 0);
}

extern "C" size_t seld_hc_conv3d_transpose_bwd_weight_workspace(const seld_conv3d_desc* d, const int32_t out_pad[3]) {
    int o[3];
    if (c3_tconv_out(d, out_pad, o) != SELD_OK) return 0;
    return c3_wgrad_bytes(g3_of(d, o, true), d->Cout, vol3(o));
}

// dw[c] += weight gradient of the mirrored convolution (x = dy, dy = x); dbias (nullable) += channel sums of dy
extern "C" int seld_hc_conv3d_transpose_bwd_weight_acc(const seld_conv3d_desc* d, const int32_t out_pad[3],
                                                       const float* x, const float* dy, float* const dw[8], float* dbias,
                                                       void* workspace, size_t workspace_bytes, void* stream) {
    int o[3];
    const int rc = c3_tconv_out(d, out_pad, o);
    if (rc) return rc;
    return c3_wgrad_run(g3_of(d, o, true), dy, x, dw, dbias, dy, d->Cout, vol3(o), workspace, workspace_bytes,
                        (hipStream_t)stream);
}

extern "C" int seld_hc_conv3d_transpose_kernel_label(const seld_conv3d_desc* d, const int32_t out_pad[3], int32_t which,
                                                     char* buf, int32_t buflen) {
    int o[3];
    const int rc = c3_tconv_out(d, out_pad, o);
    if (rc) return rc;
    if (!buf || buflen < 48 || which < 0 || which > 2) return SELD_EINVAL;
    if (which == 2) {
        snprintf(buf, buflen, "hc_conv3d_wgrad_kernel");
        return SELD_OK;
    }
    return c3_gemm_run(g3_of(d, o, which == 1), which == 0, nullptr, nullptr, nullptr, nullptr, nullptr, buf, buflen);
}
