// Hypercomplex (real / quaternion / dual-quaternion) 3-D convolution and transposed convolution, gfx950
// (F.conv3d / F.conv_transpose3d of quaternion_ops.py:125-171 and dual_quaternion_ops.py:111-153 of the reference).
//
//     conv            y[n][co][o]  = bias[co] + sum_{ci, t} x[n][ci][o*s - p + t*d] * M[co][ci][t]
//     transposed conv y[n][co][o]  = bias[co] + sum_{ci, t : o = i*s - p + t*d} u[n][ci][i] * M[ci][co][t]
//
// per axis (D, H, W); M is the Hamilton block matrix of the component tensors, read directly with the signs applied
// while staging into LDS (hc_comp), never materialised.  Three kernels serve both operations:
//
//   hc_conv3d_fwd_kernel    implicit GEMM, positions (n, od, oh, ow) x reduction (ci, td, th, tw): conv forward (+ bias),
//                           transposed-conv input gradient
//   hc_conv3d_phase_kernel  stride-phase GEMM (hc_tconv_kernel of hc_conv_transpose.hip on three axes): the output
//                           splits into sd*sh*sw residue classes; inside a class the taps that reach it form a fixed
//                           progression and the input index is an exact quotient, so each class is a dense stride-1
//                           GEMM with no per-element divisibility test and no MFMA on zeros.  Transposed-conv forward
//                           (+ bias; positions no tap reaches get the bias alone), conv input gradient
//   hc_conv3d_wgrad_kernel  G = sum dy (x) im2col(x), split over positions into a workspace of partials;
//                           hc_conv3d_fold_kernel then sums the splits in a fixed order, folds the block matrix onto the
//                           components and ADDS into dw[c] (and the bias partials into dbias)
//
// Both GEMM kernels are one body over a per-axis affine index map: output class r, phase index q (o = r + os*q), tap t
// of the class is kernel index k0[r] + t*kstep and reads input index q*im + c0[r] - t*ia.  The forward kernel is the
// single-class case (os = 1, im = stride, ia = -dil); the phase kernel has im = 1 and reads the weights transposed (the
// reduction runs over the component tensors' FIRST index, as MODE_DGRAD does).  Tiling as hc_tconv_kernel: 4 waves,
// 16*CT channels x 64*PT positions, LDS images [k/4][row][4], one ds_read_b128 feeds four v_mfma_f32_16x16x4_f32.
// For the dual quaternion a channel tile that lies in one half skips the reduction half of the zero quadrant.
//
// No float atomics anywhere: every result is run-to-run bit-identical, with or without SELD_DETERMINISTIC.
#include "hc_common.h"

namespace seld {

constexpr int C3_MAXS = 16;        // largest stride per axis (phase tables)

// one axis of the GEMM kernels' index map (see the file comment)
struct C3Axis {
    int in, out, K;
    int os, im, kstep, ia;
    int k0[C3_MAXS], n[C3_MAXS], c0[C3_MAXS], q[C3_MAXS];
};

struct C3P {
    int A, N, Cr, Co;              // reduction (streamed operand) channels, output channels
    int RA, OA;                    // Cr/A, Co/A
    int KK;                        // kd*kh*kw
    int nph;                       // residue classes: os_d*os_h*os_w
    C3Axis ax[3];
    long long x_elems;
    WPtrs w;
    const float* x;
    const float* bias;
    float* y;
};

template <int CT, int PT, bool WT>
__device__ __forceinline__ void c3_gemm(const C3P& p) {
    constexpr int BC = CT * 16;
    constexpr int BP = PT * 64;
    constexpr int XG = PT;
    constexpr int XSTEP = 256 / BP;
    constexpr int WR = (BC + 63) / 64;
    static_assert(PT == 1 || PT == 2 || PT == 4, "BP must divide 256");

    __shared__ __attribute__((aligned(16))) float Xs[2][4][BP][4];
    __shared__ __attribute__((aligned(16))) float Ws[2][4][BC][4];
    __shared__ const float* wptr_s[8];

    // ---- residue class and position tile (class fastest in the grid) ----------------------------------------
    const int ph = blockIdx.x % p.nph;
    const int tile = blockIdx.x / p.nph;
    const int rw = ph % p.ax[2].os;
    const int rdh = ph / p.ax[2].os;
    const int rh = rdh % p.ax[1].os, rd = rdh / p.ax[1].os;
    const int Qd = p.ax[0].q[rd], Qh = p.ax[1].q[rh], Qw = p.ax[2].q[rw];
    const int Qhw = Qh * Qw;
    const int PS = Qd * Qhw;                      // class positions per image
    const long long Ptot = (long long)p.N * PS;
    const long long p0 = (long long)tile * BP;
    if (p0 >= Ptot) return;                       // whole workgroup: this class has fewer tiles

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int xpos = tid & (BP - 1);
    const int xg0 = __builtin_amdgcn_readfirstlane(tid / BP);
    const int c0 = blockIdx.y * BC;
    const int KHW = p.ax[1].K * p.ax[2].K;
    const int Hi = p.ax[1].in, Wi = p.ax[2].in;
    const int Si = p.ax[0].in * Hi * Wi;

    if (tid < 8) wptr_s[tid] = p.w.p[tid];

    // reduction channel blocks; the dual quaternion's zero quadrant is M[low][high] of the component tensors' (first,
    // second) index: a low output tile of the forward reads the low reduction half only, a high output tile of the
    // phase kernel (weights transposed) the high half only
    int cb_lo = 0, cb_hi = (p.Cr + 15) >> 4;
    if (p.A == 8) {
        const int half = p.Co >> 1, rhalf = p.Cr >> 1;
        if (!WT && c0 + BC <= half) cb_hi = (rhalf + 15) >> 4;
        if (WT && c0 >= half) cb_lo = rhalf >> 4;
    }

    // taps of this class
    const int ntd = p.ax[0].n[rd], nth = p.ax[1].n[rh], ntw = p.ax[2].n[rw];
    const int nchunks = ntd * nth * ntw * (cb_hi - cb_lo);
    const int kd0 = p.ax[0].k0[rd], kh0 = p.ax[1].k0[rh], kw0 = p.ax[2].k0[rw];

    // ---- streamed operand: buffer descriptor based at the first image of the tile ----------------------------
    const long long img0 = p0 / PS;
    const long long img_elems = (long long)p.Cr * Si;
    const float* sbase = p.x + img0 * img_elems;
    const long long remain = (p.x_elems - img0 * img_elems) * 4;
    const unsigned nrec = remain > 0xFFFFFFFFLL ? 0xFFFFFFFFu : (unsigned)remain;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)sbase, 0, nrec, 0x00020000);

    // ---- this thread's staged position ------------------------------------------------------------------
    const long long pg = p0 + xpos;
    const bool pvalid = pg < Ptot;
    int bd = 0, bh = 0, bw = 0, img_b = 0;
    if (pvalid) {
        const long long n = pg / PS;
        int rem = (int)(pg - n * PS);
        const int qd = rem / Qhw;
        rem -= qd * Qhw;
        const int qh = rem / Qw;
        const int qw = rem - qh * Qw;
        bd = qd * p.ax[0].im + p.ax[0].c0[rd];
        bh = qh * p.ax[1].im + p.ax[1].c0[rh];
        bw = qw * p.ax[2].im + p.ax[2].c0[rw];
        img_b = (int)((n - img0) * img_elems * 4);
    }
    const int sib = Si * 4;

    // ---- weight rows this lane stages: output channel co -> (component, offset in component) -----------------
    int w_a[WR], w_off[WR];
    bool w_ok[WR];
#pragma unroll
    for (int j = 0; j < WR; ++j) {
        const int ch = lane + 64 * j;
        const int co = c0 + ch;
        w_ok[j] = (ch < BC) && (co < p.Co);
        const int cc = w_ok[j] ? co : 0;
        w_a[j] = cc / p.OA;
        w_off[j] = (cc - w_a[j] * p.OA) * (WT ? p.KK : p.RA * p.KK);
    }

    // ---- wave-uniform K trackers of the NEXT chunk to load: 16-channel block cb, tap (td, th, tw) ------------
    int cb = cb_lo, td = 0, th = 0, tw = 0;

    float xr[XG][4];
    float wr[WR][4], wm[WR][4];

    auto load_chunk = [&]() __attribute__((always_inline)) {
        const int ci0 = cb * 16;
        // X operand: one range check per tap, one select per element
        const int id = bd - td * p.ax[0].ia;
        const int ih = bh - th * p.ax[1].ia;
        const int iw = bw - tw * p.ax[2].ia;
        const bool ok = pvalid && ((unsigned)id < (unsigned)p.ax[0].in) && ((unsigned)ih < (unsigned)Hi) &&
                        ((unsigned)iw < (unsigned)Wi);
        const int tapb = img_b + ((id * Hi + ih) * Wi + iw) * 4;
#pragma unroll
        for (int j = 0; j < XG; ++j) {
            const int g = xg0 + j * XSTEP;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int ci = ci0 + g * 4 + s;
                const unsigned off = (ok && ci < p.Cr) ? (unsigned)(tapb + ci * sib) : 0xFFFFFFFFu;
                xr[j][s] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 0));
            }
        }
        // W operand: k-group = wave.  Loads are unconditional (an unused element reads the component's first word);
        // the sign / zero is a multiplier applied at the LDS store.
        typedef const __attribute__((address_space(1))) float* gptr;
        const int kidx = (kd0 + td * p.ax[0].kstep) * KHW + (kh0 + th * p.ax[1].kstep) * p.ax[2].K + kw0 +
                         tw * p.ax[2].kstep;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int ci = ci0 + wave * 4 + s;
            const bool kin = ci < p.Cr;
            const int cic = kin ? ci : 0;
            const int qa = cic / p.RA;
            const int cl = cic - qa * p.RA;
            const int soff = (WT ? cl * p.OA * p.KK : cl * p.KK) + kidx;
#pragma unroll
            for (int j = 0; j < WR; ++j) {
                bool zero, neg;
                const int comp = WT ? hc_comp(p.A, qa, w_a[j], &zero, &neg) : hc_comp(p.A, w_a[j], qa, &zero, &neg);
                const bool use = kin && w_ok[j] && !zero;
                gptr base = (gptr)wptr_s[comp];
                wr[j][s] = base[use ? soff + w_off[j] : 0];
                wm[j][s] = use ? (neg ? -1.f : 1.f) : 0.f;
            }
        }
        // advance: taps fastest (w, h, d), then the channel block
        if (++tw >= ntw) {
            tw = 0;
            if (++th >= nth) {
                th = 0;
                if (++td >= ntd) { td = 0; ++cb; }
            }
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

    // ---- epilogue: lane holds class positions (4 fk + r), r = 0..3, of channel fr of each 16x16 tile -------------
    const int Ho = p.ax[1].out, Wo = p.ax[2].out;
    const long long So = (long long)p.ax[0].out * Ho * Wo;
    const int osd = p.ax[0].os, osh = p.ax[1].os, osw = p.ax[2].os;
    const bool row4 = (Qw & 3) == 0;              // a lane's 4 positions lie in one class row
    const bool vec = row4 && osw == 1 && (Wo & 3) == 0;
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
                int rem = (int)(q - n * PS);
                const int qd = rem / Qhw;
                rem -= qd * Qhw;
                const int qh = rem / Qw;
                const int qw = rem - qh * Qw;
                off[r] = n * p.Co * So + ((long long)(rd + osd * qd) * Ho + rh + osh * qh) * Wo + rw + osw * qw;
            } else {
                off[r] = off[0] + r * osw;
            }
        }
#pragma unroll
        for (int j = 0; j < CT; ++j) {
            const int co = c0 + j * 16 + fr;
            if (co >= p.Co) continue;
            const float b = p.bias ? p.bias[co] : 0.f;
            const floatx4 v = acc[i][j];
            float* yc = p.y + co * So;
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

template <int CT, int PT>
__global__ __launch_bounds__(256) void hc_conv3d_fwd_kernel(const C3P p) { c3_gemm<CT, PT, false>(p); }

template <int CT, int PT>
__global__ __launch_bounds__(256) void hc_conv3d_phase_kernel(const C3P p) { c3_gemm<CT, PT, true>(p); }

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
static int c3_gcd(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

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
        if (d->stride[i] > C3_MAXS) return SELD_EUNSUPPORTED;          // phase tables
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
struct G3 {
    int A, N, Ci, Co;
    int in[3], out[3], k[3], s[3], p[3], d[3];
};

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

// forward map: one class, input index q*s - p + t*d
static void c3_axis_fwd(C3Axis& a, int s, int pad, int dil, int K, int in, int out) {
    a.in = in; a.out = out; a.K = K;
    a.os = 1; a.im = s; a.kstep = 1; a.ia = -dil;
    a.k0[0] = 0; a.n[0] = K; a.c0[0] = -pad; a.q[0] = out;
}

// stride-phase map of the transposed direction o = i*s - p + k*d (hc_conv_transpose.hip, tconv_axis)
static void c3_axis_phase(C3Axis& a, int s, int pad, int dil, int K, int in, int out) {
    const int g = c3_gcd(s, dil);
    a.in = in; a.out = out; a.K = K;
    a.os = s; a.im = 1; a.kstep = s / g; a.ia = dil / g;
    for (int r = 0; r < s; ++r) {
        int first = -1;
        for (int k = 0; k < K && k < a.kstep; ++k) {
            const int v = r + pad - k * dil;
            if (((v % s) + s) % s == 0) { first = k; break; }
        }
        if (first < 0) {
            a.k0[r] = 0; a.n[r] = 0; a.c0[r] = 0;
        } else {
            a.k0[r] = first;
            a.n[r] = (K - 1 - first) / a.kstep + 1;
            a.c0[r] = (r + pad - first * dil) / s;            // exact
        }
        a.q[r] = r < out ? (out - r + s - 1) / s : 0;
    }
}

// phase == false: y (Co, out) = conv(x (Ci, in)), weights (Co/A, Ci/A, k).
// phase == true : y (Co, out) = conv_transpose(x (Ci, in)), weights (Ci/A, Co/A, k).
static void c3_fill(C3P& p, const G3& g, bool phase, const float* const w[8]) {
    p.A = g.A; p.N = g.N; p.Cr = g.Ci; p.Co = g.Co;
    p.RA = g.Ci / g.A; p.OA = g.Co / g.A;
    p.KK = g.k[0] * g.k[1] * g.k[2];
    for (int i = 0; i < 3; ++i) {
        if (phase) c3_axis_phase(p.ax[i], g.s[i], g.p[i], g.d[i], g.k[i], g.in[i], g.out[i]);
        else c3_axis_fwd(p.ax[i], g.s[i], g.p[i], g.d[i], g.k[i], g.in[i], g.out[i]);
    }
    p.nph = p.ax[0].os * p.ax[1].os * p.ax[2].os;
    p.x_elems = (long long)g.N * g.Ci * vol3(g.in);
    for (int i = 0; i < 8; ++i) p.w.p[i] = (w && i < g.A) ? w[i] : nullptr;
}

static long long c3_class_ps(const C3P& p, int ph) {
    const int rw = ph % p.ax[2].os, rdh = ph / p.ax[2].os;
    return (long long)p.ax[0].q[rdh / p.ax[1].os] * p.ax[1].q[rdh % p.ax[1].os] * p.ax[2].q[rw];
}

// the input images a 256-position tile can touch are addressed with 32-bit byte offsets from its first image
static int c3_addressable(const C3P& p) {
    long long min_ps = 1LL << 62;
    for (int ph = 0; ph < p.nph; ++ph) {
        const long long ps = c3_class_ps(p, ph);
        if (ps > 0 && ps < min_ps) min_ps = ps;
    }
    const long long imgs = 256 / min_ps + 2;
    const long long n = imgs < p.N ? imgs : p.N;
    if (n * p.Cr * p.ax[0].in * p.ax[1].in * p.ax[2].in * 4 >= (1LL << 31)) return SELD_EUNSUPPORTED;
    return SELD_OK;
}

struct C3Cfg { int ct, pt; };

// tile choice as tconv_cfg (hc_conv_transpose.hip): fill >= 2 workgroups per CU, avoid padded channels, prefer wide tiles.
// {4, 1} serves few positions x 64 channels (a strided layer's forward): {12, 1} would pad two thirds of its channels.
static C3Cfg c3_cfg(const C3P& p) {
    static const C3Cfg cand[] = {{12, 1}, {4, 4}, {4, 1}, {2, 4}, {1, 4}};
    static const double pref[] = {1.00, 0.90, 0.60, 0.45, 0.30};
    long long P = 0;
    for (int ph = 0; ph < p.nph; ++ph) P += (long long)p.N * c3_class_ps(p, ph);
    double best = -1.0;
    C3Cfg pick = cand[1];
    for (int i = 0; i < 5; ++i) {
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
static int c3_launch(const C3P& p, bool phase, hipStream_t st) {
    constexpr int BC = CT * 16, BP = PT * 64;
    long long maxp = 0;
    for (int ph = 0; ph < p.nph; ++ph) {
        const long long pp = (long long)p.N * c3_class_ps(p, ph);
        if (pp > maxp) maxp = pp;
    }
    const long long tiles = (maxp + BP - 1) / BP;
    if (tiles * p.nph >= (1LL << 31)) return SELD_EUNSUPPORTED;
    dim3 grid((unsigned)(tiles * p.nph), (unsigned)((p.Co + BC - 1) / BC), 1);
    if (phase) hipLaunchKernelGGL((hc_conv3d_phase_kernel<CT, PT>), grid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL((hc_conv3d_fwd_kernel<CT, PT>), grid, dim3(256), 0, st, p);
    return check_launch();
}

// one GEMM launch: every check before the launch, nothing written on refusal
static int c3_gemm_run(const G3& g, bool phase, const float* x, const float* const w[8], const float* bias, float* y,
                       hipStream_t st, char* label, int buflen) {
    C3P p{};
    c3_fill(p, g, phase, w);
    int rc = c3_addressable(p);
    if (rc) return rc;
    const C3Cfg c = c3_cfg(p);
    if (label) {
        snprintf(label, buflen, "%s<%d, %d>", phase ? "hc_conv3d_phase_kernel" : "hc_conv3d_fwd_kernel", c.ct, c.pt);
        return SELD_OK;
    }
    if (!x || !w || !y) return SELD_EINVAL;
    p.x = x; p.bias = bias; p.y = y;
    if (c.ct == 12) return c3_launch<12, 1>(p, phase, st);
    if (c.ct == 4 && c.pt == 1) return c3_launch<4, 1>(p, phase, st);
    if (c.ct == 2) return c3_launch<2, 4>(p, phase, st);
    if (c.ct == 1) return c3_launch<1, 4>(p, phase, st);
    return c3_launch<4, 4>(p, phase, st);
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
