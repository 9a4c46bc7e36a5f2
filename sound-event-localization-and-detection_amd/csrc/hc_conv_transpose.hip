// Hypercomplex (real / quaternion) TRANSPOSED convolution, gfx950 (quaternion_ops.py:149-171 of the reference).
//
//     y[n][co][oh][ow] = bias[co] + sum_{ci, kh, kw} u[n][ci][ih][iw] * M[ci][co][kh][kw],
//     oh = ih*sh - ph + kh*dh,   ow = iw*sw - pw + kw*dw
//
// M (Cin, Cout, kh, kw) is the Hamilton block matrix of the component tensors (Cin/A, Cout/A, kh, kw), the same
// arrangement as the forward convolution's.  It is never materialised: signs are applied while staging into LDS.
//
// Stride-phase implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32).  The output positions split into sh*sw residue
// classes (rh, rw) = (oh mod sh, ow mod sw).  Inside a class the taps that reach it are fixed -- kh*dh == rh + ph
// (mod sh) -- and form an arithmetic progression kh = k0 + t*(sh/g), g = gcd(sh, dh); the input row of phase row qh
// (oh = rh + sh*qh) and tap t is the exact quotient ih = qh + c0 - t*(dh/g).  So each class is a dense stride-1 GEMM
// over its own tap subset: no per-element divisibility test, no MFMA on zeros, and a class with fewer taps runs
// fewer K steps.  Positions no tap reaches (a class without taps, or output_padding >= stride) get the bias only.
//
// Tiling as hc_conv_kernel (hc_conv_fwd.hip): 4 waves, BC = 16*CT output channels x BP = 64*PT phase positions; the
// LDS images are [k/4][row][4] and one ds_read_b128 feeds four MFMAs.  The K axis is (16-channel block, tap) with the
// tap fastest: consecutive K steps re-read the same 16 input channels at a shifted tap, which stay in L1.  All K
// bookkeeping is wave-uniform; the im2col gather is one tap row/column check per K step and a select per element.
//
// Stores: a lane holds 4 consecutive phase positions of one channel.  With sw == 1 they are 4 consecutive floats
// (one 16-byte store); with sw > 1 they are sw floats apart and go out as 4 dword stores.  The grid runs the phase
// index fastest, so the sw classes that interleave within one output row are resident together and their partial
// lines meet in L2 before write-back (kernel table).
//
// No float atomics: run-to-run bit-identical.
#include <type_traits>
#include "hc_common.h"

namespace seld {

constexpr int TC_MAXS = 16;        // largest stride per axis (phase tables)

struct TConvP {
    int A, N, Ci, Co, Hi, Wi, Ho, Wo;
    int KH, KW, IAt, OAt;          // IAt = Ci/A, OAt = Co/A
    int sh, sw, nph;               // nph = sh*sw
    int hstep, wstep;              // tap index step inside a class
    int ha, wa;                    // input row / column decrement per tap step
    int hk0[TC_MAXS], hn[TC_MAXS], hc0[TC_MAXS], hq[TC_MAXS];   // per H class: first tap, taps, row offset, rows
    int wk0[TC_MAXS], wn[TC_MAXS], wc0[TC_MAXS], wq[TC_MAXS];
    long long x_elems;
    WPtrs w;
    const float* x;
    const float* bias;
    float* y;
};

template <int CT, int PT>
__global__ __launch_bounds__(256) void hc_tconv_kernel(const TConvP p) {
    constexpr int BC = CT * 16;
    constexpr int BP = PT * 64;
    constexpr int XG = PT;
    constexpr int XSTEP = 256 / BP;
    constexpr int WR = (BC + 63) / 64;
    static_assert(PT == 1 || PT == 2 || PT == 4, "BP must divide 256");

    __shared__ __attribute__((aligned(16))) float Xs[2][4][BP][4];
    __shared__ __attribute__((aligned(16))) float Ws[2][4][BC][4];
    __shared__ const float* wptr_s[8];

    // ---- phase class and position tile (phase fastest in the grid) ----------------------------------------
    const int ph = blockIdx.x % p.nph;
    const int tile = blockIdx.x / p.nph;
    const int rh = ph / p.sw, rw = ph - rh * p.sw;
    const int Qh = p.hq[rh], Qw = p.wq[rw];
    const int PS = Qh * Qw;                       // phase positions per image
    const long long Ptot = (long long)p.N * PS;
    const long long p0 = (long long)tile * BP;
    if (p0 >= Ptot) return;                       // whole workgroup: this class has fewer tiles

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int xpos = tid & (BP - 1);
    const int xg0 = __builtin_amdgcn_readfirstlane(tid / BP);
    const int c0 = blockIdx.y * BC;
    const int KK = p.KH * p.KW;
    const int HWi = p.Hi * p.Wi;

    if (tid < 8) wptr_s[tid] = p.w.p[tid];

    // taps of this class
    const int nth = p.hn[rh], ntw = p.wn[rw];
    const int T = nth * ntw;
    const int ncb = (p.Ci + 15) >> 4;
    const int nchunks = T * ncb;
    const int kh0 = p.hk0[rh], kw0 = p.wk0[rw];

    // ---- streamed operand: buffer descriptor based at the first image of the tile ----------------------------
    const long long img0 = p0 / PS;
    const long long img_elems = (long long)p.Ci * HWi;
    const float* sbase = p.x + img0 * img_elems;
    const long long remain = (p.x_elems - img0 * img_elems) * 4;
    const unsigned nrec = remain > 0xFFFFFFFFLL ? 0xFFFFFFFFu : (unsigned)remain;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)sbase, 0, nrec, 0x00020000);

    // ---- this thread's staged position ------------------------------------------------------------------
    const long long pg = p0 + xpos;
    const bool pvalid = pg < Ptot;
    int base_h = 0, base_w = 0, img_b = 0;
    if (pvalid) {
        const long long n = pg / PS;
        const int rem = (int)(pg - n * PS);
        const int qh = rem / Qw;
        const int qw = rem - qh * Qw;
        base_h = qh + p.hc0[rh];
        base_w = qw + p.wc0[rw];
        img_b = (int)(n - img0) * (int)img_elems * 4;
    }
    const int hwb = HWi * 4;

    // ---- weight rows this lane stages: output channel co -> (component, index in component) ------------------
    int w_a[WR], w_off[WR];
    bool w_ok[WR];
#pragma unroll
    for (int j = 0; j < WR; ++j) {
        const int ch = lane + 64 * j;
        const int co = c0 + ch;
        w_ok[j] = (ch < BC) && (co < p.Co);
        const int cc = w_ok[j] ? co : 0;
        w_a[j] = cc / p.OAt;
        w_off[j] = (cc - w_a[j] * p.OAt) * KK;
    }

    // ---- wave-uniform K trackers of the NEXT chunk to load: 16-channel block cb, tap (th, tw) ----------------
    int cb = 0, th = 0, tw = 0;

    float xr[XG][4];
    float wr[WR][4], wm[WR][4];

    auto load_chunk = [&]() __attribute__((always_inline)) {
        const int ci0 = cb * 16;
        // X operand: one range check per tap, one select per element
        const int ih = base_h - th * p.ha;
        const int iw = base_w - tw * p.wa;
        const bool ok = pvalid && ((unsigned)ih < (unsigned)p.Hi) && ((unsigned)iw < (unsigned)p.Wi);
        const int tapb = img_b + (ih * p.Wi + iw) * 4;
#pragma unroll
        for (int j = 0; j < XG; ++j) {
            const int g = xg0 + j * XSTEP;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int ci = ci0 + g * 4 + s;
                const unsigned off = (ok && ci < p.Ci) ? (unsigned)(tapb + ci * hwb) : 0xFFFFFFFFu;
                xr[j][s] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 0));
            }
        }
        // W operand: k-group = wave; M[ci][co][kidx] = sign * W_comp[ci_l][co_l][kidx].  Loads are unconditional (an
        // unused element reads the component's first word); the sign / zero is a multiplier applied at the LDS store.
        typedef const __attribute__((address_space(1))) float* gptr;
        const int kidx = (kh0 + th * p.hstep) * p.KW + kw0 + tw * p.wstep;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int ci = ci0 + wave * 4 + s;
            const bool kin = ci < p.Ci;
            const int cic = kin ? ci : 0;
            const int qa = cic / p.IAt;
            const int soff = (cic - qa * p.IAt) * p.OAt * KK + kidx;
#pragma unroll
            for (int j = 0; j < WR; ++j) {
                bool zero, neg;
                const int comp = hc_comp(p.A, qa, w_a[j], &zero, &neg);
                const bool use = kin && w_ok[j] && !zero;
                gptr base = (gptr)wptr_s[comp];
                wr[j][s] = base[use ? soff + w_off[j] : 0];
                wm[j][s] = use ? (neg ? -1.f : 1.f) : 0.f;
            }
        }
        // advance: tap fastest, then the channel block
        if (++tw >= ntw) {
            tw = 0;
            if (++th >= nth) { th = 0; ++cb; }
        }
    };
    auto store_chunk = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < XG; ++j)
            *reinterpret_cast<float4*>(&Xs[buf][xg0 + j * XSTEP][xpos][0]) = make_float4(xr[j][0], xr[j][1], xr[j][2], xr[j][3]);
#pragma unroll
        for (int j = 0; j < WR; ++j) {
            const int ch = lane + 64 * j;
            if (ch < BC)
                *reinterpret_cast<float4*>(&Ws[buf][wave][ch][0]) =
                    make_float4(wr[j][0] * wm[j][0], wr[j][1] * wm[j][1], wr[j][2] * wm[j][2], wr[j][3] * wm[j][3]);
        }
    };

    floatx4 acc[PT][CT];
#pragma unroll
    for (int i = 0; i < PT; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j) acc[i][j] = (floatx4){0.f, 0.f, 0.f, 0.f};

    const int fr = lane & 15;
    const int fk = lane >> 4;

    __syncthreads();               // wptr_s visible
    if (nchunks > 0) {
        load_chunk();
        store_chunk(0);
    }
    __syncthreads();
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        const int buf = chunk & 1;
        if (chunk + 1 < nchunks) load_chunk();
        float av[PT][4], bv[CT][4];
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            const float4 t = *reinterpret_cast<const float4*>(&Xs[buf][fk][wave * (PT * 16) + i * 16 + fr][0]);
            av[i][0] = t.x; av[i][1] = t.y; av[i][2] = t.z; av[i][3] = t.w;
        }
#pragma unroll
        for (int j = 0; j < CT; ++j) {
            const float4 t = *reinterpret_cast<const float4*>(&Ws[buf][fk][j * 16 + fr][0]);
            bv[j][0] = t.x; bv[j][1] = t.y; bv[j][2] = t.z; bv[j][3] = t.w;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int j = 0; j < CT; ++j)
#pragma unroll
                for (int i = 0; i < PT; ++i)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][s], bv[j][s], acc[i][j], 0, 0, 0);
        if (chunk + 1 < nchunks) store_chunk(buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue: lane holds phase positions (4 fk + r), r = 0..3, of channel fr of each 16x16 tile -------------
    const long long HWo = (long long)p.Ho * p.Wo;
    const bool row4 = (Qw & 3) == 0;              // a lane's 4 positions lie in one phase row
    const bool vec = row4 && p.sw == 1 && (p.Wo & 3) == 0;
#pragma unroll
    for (int i = 0; i < PT; ++i) {
        const long long pos = p0 + wave * (PT * 16) + i * 16 + fk * 4;
        long long off[4];
        bool ok[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long long q = pos + r;
            ok[r] = q < Ptot;
            if (r == 0 || !row4) {
                const long long n = ok[r] ? q / PS : 0;
                const int rem = (int)(q - n * PS);
                const int qh = rem / Qw;
                const int qw = rem - qh * Qw;
                off[r] = n * p.Co * HWo + (long long)(rh + p.sh * qh) * p.Wo + rw + p.sw * qw;
            } else {
                off[r] = off[0] + r * p.sw;
            }
        }
#pragma unroll
        for (int j = 0; j < CT; ++j) {
            const int co = c0 + j * 16 + fr;
            if (co >= p.Co) continue;
            const float b = p.bias ? p.bias[co] : 0.f;
            const floatx4 v = acc[i][j];
            float* yc = p.y + co * HWo;
            if (vec && ok[0]) {
                *reinterpret_cast<float4*>(yc + off[0]) = make_float4(v[0] + b, v[1] + b, v[2] + b, v[3] + b);
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (ok[r]) yc[off[r]] = v[r] + b;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct TCfg { int ct, pt; };

static int gcd_i(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

// Output extent per axis: (in - 1)*s - 2p + d*(k - 1) + op + 1; PyTorch's rule: op < s or op < d.
static int tconv_validate(const seld_conv_desc* d, const int32_t op[2], int out[2]) {
    int rc = hc_validate(d);
    if (rc) return rc;
    if (!op) return SELD_EINVAL;
    for (int i = 0; i < 2; ++i) {
        if (op[i] < 0 || (op[i] >= d->stride[i] && op[i] >= d->dil[i])) return SELD_EINVAL;
        out[i] = (d->in[i] - 1) * d->stride[i] - 2 * d->pad[i] + d->dil[i] * (d->k[i] - 1) + op[i] + 1;
        if (out[i] <= 0) return SELD_EINVAL;
    }
    if (d->ndim == 1 && (d->in[0] != 1 || d->k[0] != 1 || d->stride[0] != 1 || d->pad[0] != 0 || op[0] != 0))
        return SELD_EINVAL;
    return SELD_OK;
}

// Limits of the phase kernel's addressing: per-axis stride <= TC_MAXS (phase tables), one output image addressed with
// 32-bit offsets like the input, and the input images one tile spans addressed with 32-bit byte offsets.
static int tconv_addressable(const seld_conv_desc* d, const int out[2]) {
    if (d->algebra == 8) return SELD_EUNSUPPORTED;            // no dual-quaternion transposed convolution in the reference
    if (d->stride[0] > TC_MAXS || d->stride[1] > TC_MAXS) return SELD_EUNSUPPORTED;
    if ((long long)d->Cout * out[0] * out[1] >= (1LL << 28)) return SELD_EUNSUPPORTED;
    long long min_ps = 1LL << 62;
    for (int rh = 0; rh < d->stride[0]; ++rh)
        for (int rw = 0; rw < d->stride[1]; ++rw) {
            const long long qh = rh < out[0] ? (out[0] - rh + d->stride[0] - 1) / d->stride[0] : 0;
            const long long qw = rw < out[1] ? (out[1] - rw + d->stride[1] - 1) / d->stride[1] : 0;
            if (qh * qw > 0 && qh * qw < min_ps) min_ps = qh * qw;
        }
    const long long imgs = 256 / min_ps + 2;                  // images a 256-position tile can touch
    const long long n = imgs < d->N ? imgs : d->N;
    if (n * d->Cin * d->in[0] * d->in[1] * 4 >= (1LL << 31)) return SELD_EUNSUPPORTED;
    return SELD_OK;
}

static void tconv_axis(int s, int pad, int dil, int K, int in, int out, int* k0, int* n, int* c0, int* q, int* step,
                       int* a) {
    const int g = gcd_i(s, dil);
    *step = s / g;
    *a = dil / g;
    for (int r = 0; r < s; ++r) {
        int first = -1;
        for (int k = 0; k < K && k < *step; ++k) {
            const int v = r + pad - k * dil;
            if (((v % s) + s) % s == 0) { first = k; break; }
        }
        if (first < 0) {
            k0[r] = 0; n[r] = 0; c0[r] = 0;
        } else {
            k0[r] = first;
            n[r] = (K - 1 - first) / *step + 1;
            c0[r] = (r + pad - first * dil) / s;             // exact
        }
        q[r] = r < out ? (out - r + s - 1) / s : 0;
    }
    (void)in;
}

static void tconv_fill(TConvP& p, const seld_conv_desc* d, const int out[2], const float* const w[8]) {
    p.A = d->algebra; p.N = d->N; p.Ci = d->Cin; p.Co = d->Cout;
    p.Hi = d->in[0]; p.Wi = d->in[1]; p.Ho = out[0]; p.Wo = out[1];
    p.KH = d->k[0]; p.KW = d->k[1];
    p.IAt = d->Cin / d->algebra; p.OAt = d->Cout / d->algebra;
    p.sh = d->stride[0]; p.sw = d->stride[1]; p.nph = p.sh * p.sw;
    tconv_axis(p.sh, d->pad[0], d->dil[0], p.KH, p.Hi, p.Ho, p.hk0, p.hn, p.hc0, p.hq, &p.hstep, &p.ha);
    tconv_axis(p.sw, d->pad[1], d->dil[1], p.KW, p.Wi, p.Wo, p.wk0, p.wn, p.wc0, p.wq, &p.wstep, &p.wa);
    p.x_elems = (long long)d->N * d->Cin * d->in[0] * d->in[1];
    for (int i = 0; i < 8; ++i) p.w.p[i] = (w && i < d->algebra) ? w[i] : nullptr;
}

// Tile choice as pick_cfg (hc_conv_fwd.hip): fill >= 2 workgroups per CU, avoid padded channels, prefer wide tiles.
static TCfg tconv_cfg(const TConvP& p) {
    static const TCfg cand[] = {{12, 1}, {4, 4}, {2, 4}, {1, 4}};
    static const double pref[] = {1.00, 0.90, 0.45, 0.30};
    long long P = 0;
    for (int ph = 0; ph < p.nph; ++ph) P += (long long)p.N * p.hq[ph / p.sw] * p.wq[ph % p.sw];
    double best = -1.0;
    TCfg pick = cand[1];
    for (int i = 0; i < 4; ++i) {
        const int bc = cand[i].ct * 16, bp = cand[i].pt * 64;
        const long long cb = (p.Co + bc - 1) / bc;
        const long long wgs = ((P + bp - 1) / bp) * cb;
        const double fill = wgs >= 512 ? 1.0 : (double)wgs / 512.0;
        const double use = (double)p.Co / (double)(cb * bc);
        const double score = fill * use * pref[i];
        if (score > best) { best = score; pick = cand[i]; }
    }
    return pick;
}

template <int CT, int PT>
static int tconv_launch(const TConvP& p, hipStream_t st) {
    constexpr int BC = CT * 16, BP = PT * 64;
    long long maxp = 0;
    for (int ph = 0; ph < p.nph; ++ph) {
        const long long pp = (long long)p.N * p.hq[ph / p.sw] * p.wq[ph % p.sw];
        if (pp > maxp) maxp = pp;
    }
    const long long tiles = (maxp + BP - 1) / BP;
    if (tiles * p.nph >= (1LL << 31)) return SELD_EUNSUPPORTED;
    dim3 grid((unsigned)(tiles * p.nph), (unsigned)((p.Co + BC - 1) / BC), 1);
    hipLaunchKernelGGL((hc_tconv_kernel<CT, PT>), grid, dim3(256), 0, st, p);
    return check_launch();
}

// Reduction over batch and positions of dy (N, C, S) per channel, added to out[c]: one workgroup per channel, fixed order.
__global__ __launch_bounds__(256) void tconv_bias_grad_kernel(const float* __restrict__ dy, int N, int C, long long S,
                                                              float* __restrict__ out) {
    const int c = blockIdx.x;
    float s = 0.f;
    for (int n = 0; n < N; ++n) {
        const float* row = dy + ((size_t)n * C + c) * S;
        for (long long i = threadIdx.x; i < S; i += 256) s += row[i];
    }
    __shared__ float red[4];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[c] += red[0] + red[1] + red[2] + red[3];
}

// the mirrored convolution: input = the transposed convolution's output, output = its input, same component tensors
static seld_conv_desc tconv_mirror(const seld_conv_desc* d, const int out[2]) {
    seld_conv_desc m = *d;
    m.Cin = d->Cout; m.Cout = d->Cin;
    m.in[0] = out[0]; m.in[1] = out[1];
    return m;
}

}  // namespace seld

using namespace seld;

extern "C" int seld_hc_conv_transpose_out_shape(const seld_conv_desc* d, const int32_t out_pad[2], int32_t out[2]) {
    int o[2];
    const int rc = tconv_validate(d, out_pad, o);
    if (rc) return rc;
    if (out) { out[0] = o[0]; out[1] = o[1]; }
    return SELD_OK;
}

extern "C" int seld_hc_conv_transpose_fwd(const seld_conv_desc* d, const int32_t out_pad[2], const float* x,
                                          const float* const w[8], const float* bias, float* y, void* stream) {
    int o[2];
    int rc = tconv_validate(d, out_pad, o);
    if (rc) return rc;
    if (!x || !w || !y) return SELD_EINVAL;
    rc = tconv_addressable(d, o);
    if (rc) return rc;
    TConvP p{};
    tconv_fill(p, d, o, w);
    p.x = x; p.bias = bias; p.y = y;
    const TCfg c = tconv_cfg(p);
    hipStream_t st = (hipStream_t)stream;
    if (c.ct == 12) return tconv_launch<12, 1>(p, st);
    if (c.ct == 2) return tconv_launch<2, 4>(p, st);
    if (c.ct == 1) return tconv_launch<1, 4>(p, st);
    return tconv_launch<4, 4>(p, st);
}

// dx = conv(dy, M) with the same stride / padding / dilation, cut to the transposed convolution's input extent
extern "C" int seld_hc_conv_transpose_bwd_data(const seld_conv_desc* d, const int32_t out_pad[2], const float* dy,
                                               const float* const w[8], float* dx, void* stream) {
    int o[2];
    int rc = tconv_validate(d, out_pad, o);
    if (rc) return rc;
    if (!dy || !w || !dx) return SELD_EINVAL;
    rc = tconv_addressable(d, o);
    if (rc) return rc;
    const seld_conv_desc m = tconv_mirror(d, o);
    return hc_conv_fwd_out(&m, d->in, dy, w, dx, (hipStream_t)stream);
}

extern "C" size_t seld_hc_conv_transpose_bwd_weight_workspace(const seld_conv_desc* d, const int32_t out_pad[2]) {
    int o[2];
    if (tconv_validate(d, out_pad, o) != SELD_OK || !env().deterministic) return 0;
    return (size_t)d->Cout * d->Cin * d->k[0] * d->k[1] * sizeof(float);
}

// dw[c] += weight gradient of the mirrored convolution with x = dy and dy = x; dbias (nullable) += sum of dy
extern "C" int seld_hc_conv_transpose_bwd_weight_acc(const seld_conv_desc* d, const int32_t out_pad[2], const float* x,
                                                     const float* dy, float* const dw[8], float* dbias, void* workspace,
                                                     size_t workspace_bytes, void* stream) {
    int o[2];
    int rc = tconv_validate(d, out_pad, o);
    if (rc) return rc;
    if (!x || !dy || !dw) return SELD_EINVAL;
    rc = tconv_addressable(d, o);
    if (rc) return rc;
    if (workspace_bytes < seld_hc_conv_transpose_bwd_weight_workspace(d, out_pad)) return SELD_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const seld_conv_desc m = tconv_mirror(d, o);
    rc = hc_wgrad_out(&m, d->in, dy, x, dw, workspace, workspace_bytes, st);
    if (rc) return rc;
    if (dbias) {
        hipLaunchKernelGGL(tconv_bias_grad_kernel, dim3(d->Cout), dim3(256), 0, st, dy, d->N, d->Cout,
                           (long long)o[0] * o[1], dbias);
        rc = check_launch();
    }
    return rc;
}

// Kernel symbol a call would launch: which = 0 forward, 1 input gradient, 2 weight gradient.
extern "C" int seld_hc_conv_transpose_kernel_label(const seld_conv_desc* d, const int32_t out_pad[2], int32_t which,
                                                   char* buf, int32_t buflen) {
    int o[2];
    int rc = tconv_validate(d, out_pad, o);
    if (rc || !buf || buflen < 48) return rc ? rc : SELD_EINVAL;
    if (which == 1 || which == 2) {
        const seld_conv_desc m = tconv_mirror(d, o);
        return seld_hc_conv_kernel_label(&m, which == 1 ? 0 : 2, buf, buflen);
    }
    TConvP p{};
    tconv_fill(p, d, o, nullptr);
    const TCfg c = tconv_cfg(p);
    snprintf(buf, buflen, "hc_tconv_kernel<%d, %d>", c.ct, c.pt);
    return SELD_OK;
}
