// The stride-phase / forward implicit GEMM of the transposed and 3-D convolutions on NAX spatial axes (hc_conv_transpose.hip:
// NAX = 2; hc_conv3d.hip: NAX = 3), gfx950: one device body and one host plan.  Each file instantiates its own kernels.
//
// One body over a per-axis affine index map: output class r, phase index q (o = r + os*q); tap t of the class is kernel
// index k0[r] + t*kstep and reads input index q*im + c0[r] - t*ia.
//
//   forward map  one class per axis: os = 1, im = stride, ia = -dil, every tap.
//                y[co][o] = bias[co] + sum_{ci, t} x[ci][o*s - p + t*d] * M[co][ci][t]
//   phase map    the transposed direction o = i*s - p + k*d.  The output positions split into prod(s) residue classes
//                r = o mod s per axis.  Inside a class the taps that reach it are fixed -- k*d == r + p (mod s) -- and form
//                an arithmetic progression k = k0 + t*(s/g), g = gcd(s, d); the input index of phase index q and tap t is
//                the exact quotient q + c0 - t*(d/g).  So each class is a dense stride-1 GEMM over its own tap subset: no
//                per-element divisibility test, no MFMA on zeros, and a class with fewer taps runs fewer K steps.
//                Positions no tap reaches (a class without taps, or output_padding >= stride) get the bias only.
//                y[co][o] = bias[co] + sum_{ci, t : o = i*s - p + t*d} u[ci][i] * M[ci][co][t]
//
// M is the Hamilton block matrix of the component tensors.  It is never materialised: signs are applied while staging
// into LDS (hc_comp).  WT: the reduction runs over the component tensors' FIRST index (weights read transposed, as
// MODE_DGRAD does); the phase map is used with WT = true, the forward map with WT = false.  For the dual quaternion a
// channel tile that lies in one half skips the reduction half of the zero quadrant.
//
// Tiling as hc_conv_kernel (hc_conv_fwd.hip): 4 waves, BC = 16*CT output channels x BP = 64*PT class positions; the LDS
// images are [k/4][row][4] and one ds_read_b128 feeds four v_mfma_f32_16x16x4_f32 (exact fp32).  The K axis is
// (16-channel block, tap) with the tap fastest (last axis first): consecutive K steps re-read the same 16 input channels
// at a shifted tap, which stay in L1.  All K bookkeeping is wave-uniform; the im2col gather is one range check per K step
// and a select per element.
//
// Stores: a lane holds 4 consecutive class positions of one channel.  With os == 1 on the last axis they are 4
// consecutive floats (one 16-byte store); with os > 1 they are os floats apart and go out as 4 dword stores.  The grid
// runs the class index fastest, so the classes that interleave within one output row are resident together and their
// partial lines meet in L2 before write-back (kernel table).
//
// No float atomics: run-to-run bit-identical.
#pragma once
#include "hc_common.h"

namespace seld {

constexpr int PG_MAXS = 16;        // largest stride per axis (phase tables)

// one axis of the index map
struct PgAxis {
    int in, out, K;
    int os, im, kstep, ia;
    int k0[PG_MAXS], n[PG_MAXS], c0[PG_MAXS], q[PG_MAXS];    // per class: first tap, taps, input offset, phase extent
};

template <int NAX>
struct PgP {
    int A, N, Cr, Co;              // reduction (streamed operand) channels, output channels
    int RA, OA;                    // Cr/A, Co/A
    int KK;                        // taps: product of the kernel extents
    int nph;                       // residue classes: product of os
    PgAxis ax[NAX];                // slowest axis first
    long long x_elems;
    WPtrs w;
    const float* x;
    const float* bias;
    float* y;
};

template <int CT, int PT, bool WT, int NAX>
__device__ __forceinline__ void pg_gemm(const PgP<NAX>& p) {
    constexpr int BC = CT * 16;
    constexpr int BP = PT * 64;
    constexpr int XG = PT;
    constexpr int XSTEP = 256 / BP;
    constexpr int WR = (BC + 63) / 64;
    constexpr int L = NAX - 1;     // the contiguous axis
    static_assert(PT == 1 || PT == 2 || PT == 4, "BP must divide 256");
    static_assert(NAX == 2 || NAX == 3, "axes");

    __shared__ __attribute__((aligned(16))) float Xs[2][4][BP][4];
    __shared__ __attribute__((aligned(16))) float Ws[2][4][BC][4];
    __shared__ const float* wptr_s[8];

    // ---- residue class and position tile (class fastest in the grid) ----------------------------------------
    const int ph = blockIdx.x % p.nph;
    const int tile = blockIdx.x / p.nph;
    int r[NAX], Q[NAX];
    {
        int rest = ph;
#pragma unroll
        for (int a = L; a > 0; --a) {
            const int hi = rest / p.ax[a].os;
            r[a] = rest - hi * p.ax[a].os;
            rest = hi;
        }
        r[0] = rest;
    }
#pragma unroll
    for (int a = 0; a < NAX; ++a) Q[a] = p.ax[a].q[r[a]];
    int Qin[NAX];                                 // class positions per step of axis a: product of Q[b], b > a
    Qin[L] = 1;
#pragma unroll
    for (int a = L; a > 0; --a) Qin[a - 1] = Qin[a] * Q[a];
    const int PS = Q[0] * Qin[0];                 // class positions per image
    const long long Ptot = (long long)p.N * PS;
    const long long p0 = (long long)tile * BP;
    if (p0 >= Ptot) return;                       // whole workgroup: this class has fewer tiles

    // class position inside an image -> phase index per axis
    auto split = [&](int rem, int (&q)[NAX]) __attribute__((always_inline)) {
#pragma unroll
        for (int a = 0; a < L; ++a) {
            q[a] = rem / Qin[a];
            rem -= q[a] * Qin[a];
        }
        q[L] = rem;
    };

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int xpos = tid & (BP - 1);
    const int xg0 = __builtin_amdgcn_readfirstlane(tid / BP);
    const int c0 = blockIdx.y * BC;
    int Si = 1;
#pragma unroll
    for (int a = 0; a < NAX; ++a) Si *= p.ax[a].in;

    if (tid < 8) wptr_s[tid] = p.w.p[tid];

    // reduction channel blocks; the dual quaternion's zero quadrant is M[low][high] of the component tensors' (first,
    // second) index: a low output tile of the forward reads the low reduction half only, a high output tile of the
    // transposed read the high half only
    int cb_lo = 0, cb_hi = (p.Cr + 15) >> 4;
    if (p.A == 8) {
        const int half = p.Co >> 1, rhalf = p.Cr >> 1;
        if (!WT && c0 + BC <= half) cb_hi = (rhalf + 15) >> 4;
        if (WT && c0 >= half) cb_lo = rhalf >> 4;
    }

    // taps of this class: tap t[] is kernel element kbase + sum t[a]*kinc[a] of a component tensor
    int nt[NAX], kinc[NAX];
    int nchunks = cb_hi - cb_lo, kbase = 0, kstride = 1;
#pragma unroll
    for (int a = L; a >= 0; --a) {
        nt[a] = p.ax[a].n[r[a]];
        nchunks *= nt[a];
        kbase += p.ax[a].k0[r[a]] * kstride;
        kinc[a] = p.ax[a].kstep * kstride;
        kstride *= p.ax[a].K;
    }

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
    int base[NAX], img_b = 0;
#pragma unroll
    for (int a = 0; a < NAX; ++a) base[a] = 0;
    if (pvalid) {
        const long long n = pg / PS;
        int q[NAX];
        split((int)(pg - n * PS), q);
#pragma unroll
        for (int a = 0; a < NAX; ++a) base[a] = q[a] * p.ax[a].im + p.ax[a].c0[r[a]];
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

    // ---- wave-uniform K trackers of the NEXT chunk to load: 16-channel block cb, tap t[] per axis ------------
    int cb = cb_lo, t[NAX];
#pragma unroll
    for (int a = 0; a < NAX; ++a) t[a] = 0;

    float xr[XG][4];
    float wr[WR][4], wm[WR][4];

    auto load_chunk = [&]() __attribute__((always_inline)) {
        const int ci0 = cb * 16;
        // X operand: one range check per tap, one select per element.  `&`, not `&&`: with the short-circuit form the
        // compiler branches on `ok` around the first chunk's loads (2 to 4 more VGPRs in the PT = 4 instantiations)
        bool ok = pvalid;
        int lin = 0, kidx = kbase;
#pragma unroll
        for (int a = 0; a < NAX; ++a) {
            const int i = base[a] - t[a] * p.ax[a].ia;
            ok &= (unsigned)i < (unsigned)p.ax[a].in;
            lin = lin * p.ax[a].in + i;
            kidx += t[a] * kinc[a];
        }
        const int tapb = img_b + lin * 4;
#pragma unroll
        for (int j = 0; j < XG; ++j) {
            const int g = xg0 + j * XSTEP;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int ci = ci0 + g * 4 + s;
                const unsigned off = (ok & (ci < p.Cr)) ? (unsigned)(tapb + ci * sib) : 0xFFFFFFFFu;
                xr[j][s] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, off, 0, 0));
            }
        }
        // W operand: k-group = wave.  Loads are unconditional (an unused element reads the component's first word);
        // the sign / zero is a multiplier applied at the LDS store.
        typedef const __attribute__((address_space(1))) float* gptr;
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
                gptr wbase = (gptr)wptr_s[comp];
                wr[j][s] = wbase[use ? soff + w_off[j] : 0];
                wm[j][s] = use ? (neg ? -1.f : 1.f) : 0.f;
            }
        }
        // advance: taps fastest (last axis first), then the channel block.  The early exit keeps this a nest of scalar
        // branches; a carry flag through all axes cost the 3-D PT = 4 instantiations 2 VGPRs
#pragma unroll
        for (int a = L; a >= 0; --a) {
            if (++t[a] < nt[a]) break;
            t[a] = 0;
            if (a == 0) ++cb;
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
            const float4 f = *reinterpret_cast<const float4*>(&Xs[buf][fk][wave * (PT * 16) + i * 16 + fr][0]);
            av[i][0] = f.x; av[i][1] = f.y; av[i][2] = f.z; av[i][3] = f.w;
        }
#pragma unroll
        for (int j = 0; j < CT; ++j) {
            const float4 f = *reinterpret_cast<const float4*>(&Ws[buf][fk][j * 16 + fr][0]);
            bv[j][0] = f.x; bv[j][1] = f.y; bv[j][2] = f.z; bv[j][3] = f.w;
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

    // ---- epilogue: lane holds class positions (4 fk + e), e = 0..3, of channel fr of each 16x16 tile -------------
    long long So = 1;
#pragma unroll
    for (int a = 0; a < NAX; ++a) So *= p.ax[a].out;
    const int osw = p.ax[L].os;
    const bool row4 = (Q[L] & 3) == 0;            // a lane's 4 positions lie in one class row
    const bool vec = row4 && osw == 1 && (p.ax[L].out & 3) == 0;
#pragma unroll
    for (int i = 0; i < PT; ++i) {
        const long long pos = p0 + wave * (PT * 16) + i * 16 + fk * 4;
        long long off[4];
        bool ok[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long long pq = pos + e;
            ok[e] = pq < Ptot;
            if (e == 0 || !row4) {
                const long long n = ok[e] ? pq / PS : 0;
                int q[NAX];
                split((int)(pq - n * PS), q);
                long long o = r[0] + p.ax[0].os * q[0];
#pragma unroll
                for (int a = 1; a < NAX; ++a) o = o * p.ax[a].out + r[a] + p.ax[a].os * q[a];
                off[e] = n * p.Co * So + o;
            } else {
                off[e] = off[0] + e * osw;
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
                for (int e = 0; e < 4; ++e)
                    if (ok[e]) yc[off[e]] = v[e] + b;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// host plan
// ------------------------------------------------------------------------------------------
// geometry of one launch in convolution terms: x (Ci, in) -> y (Co, out)
template <int NAX>
struct PgGeom {
    int A, N, Ci, Co;
    int in[NAX], out[NAX], k[NAX], s[NAX], p[NAX], d[NAX];
};

inline int pg_gcd(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

// forward map: one class, input index q*s - p + t*d
inline void pg_axis_fwd(PgAxis& a, int s, int pad, int dil, int K, int in, int out) {
    a.in = in; a.out = out; a.K = K;
    a.os = 1; a.im = s; a.kstep = 1; a.ia = -dil;
    a.k0[0] = 0; a.n[0] = K; a.c0[0] = -pad; a.q[0] = out;
}

// stride-phase map of the transposed direction o = i*s - p + k*d; s <= PG_MAXS
inline void pg_axis_phase(PgAxis& a, int s, int pad, int dil, int K, int in, int out) {
    const int g = pg_gcd(s, dil);
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
template <int NAX>
inline void pg_fill(PgP<NAX>& p, const PgGeom<NAX>& g, bool phase, const float* const w[8]) {
    p.A = g.A; p.N = g.N; p.Cr = g.Ci; p.Co = g.Co;
    p.RA = g.Ci / g.A; p.OA = g.Co / g.A;
    p.KK = 1; p.nph = 1;
    p.x_elems = (long long)g.N * g.Ci;
    for (int i = 0; i < NAX; ++i) {
        if (phase) pg_axis_phase(p.ax[i], g.s[i], g.p[i], g.d[i], g.k[i], g.in[i], g.out[i]);
        else pg_axis_fwd(p.ax[i], g.s[i], g.p[i], g.d[i], g.k[i], g.in[i], g.out[i]);
        p.KK *= g.k[i];
        p.nph *= p.ax[i].os;
        p.x_elems *= g.in[i];
    }
    for (int i = 0; i < 8; ++i) p.w.p[i] = (w && i < g.A) ? w[i] : nullptr;
}

// positions per image of residue class ph
template <int NAX>
inline long long pg_class_ps(const PgP<NAX>& p, int ph) {
    long long ps = 1;
    for (int a = NAX - 1; a >= 0; --a) {
        ps *= p.ax[a].q[ph % p.ax[a].os];
        ph /= p.ax[a].os;
    }
    return ps;
}

// the input images a 256-position tile can touch are addressed with 32-bit byte offsets from its first image
template <int NAX>
inline int pg_addressable(const PgP<NAX>& p) {
    long long min_ps = 1LL << 62;
    for (int ph = 0; ph < p.nph; ++ph) {
        const long long ps = pg_class_ps(p, ph);
        if (ps > 0 && ps < min_ps) min_ps = ps;
    }
    const long long imgs = 256 / min_ps + 2;
    long long bytes = (imgs < p.N ? imgs : p.N) * p.Cr * 4;
    for (int a = 0; a < NAX; ++a) bytes *= p.ax[a].in;
    return bytes >= (1LL << 31) ? SELD_EUNSUPPORTED : SELD_OK;
}

struct PgCfg { int ct, pt; };

// Tile choice as pick_cfg (hc_conv_fwd.hip): fill >= 2 workgroups per CU, avoid padded channels, prefer wide tiles.
// {4, 1} (narrow == true only) serves few positions x 64 channels (a strided 3-D layer's forward): {12, 1} would pad two
// thirds of its channels.
template <int NAX>
inline PgCfg pg_cfg(const PgP<NAX>& p, bool narrow) {
    static const PgCfg cand[] = {{12, 1}, {4, 4}, {4, 1}, {2, 4}, {1, 4}};
    static const double pref[] = {1.00, 0.90, 0.60, 0.45, 0.30};
    long long P = 0;
    for (int ph = 0; ph < p.nph; ++ph) P += (long long)p.N * pg_class_ps(p, ph);
    double best = -1.0;
    PgCfg pick = cand[1];
    for (int i = 0; i < 5; ++i) {
        if (i == 2 && !narrow) continue;
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

// kern: the caller's instantiation for tile c
template <int NAX>
inline int pg_launch(void (*kern)(const PgP<NAX>), PgCfg c, const PgP<NAX>& p, hipStream_t st) {
    const int bc = c.ct * 16, bp = c.pt * 64;
    long long maxp = 0;
    for (int ph = 0; ph < p.nph; ++ph) {
        const long long pp = (long long)p.N * pg_class_ps(p, ph);
        if (pp > maxp) maxp = pp;
    }
    const long long tiles = (maxp + bp - 1) / bp;
    if (tiles * p.nph >= (1LL << 31)) return SELD_EUNSUPPORTED;
    dim3 grid((unsigned)(tiles * p.nph), (unsigned)((p.Co + bc - 1) / bc), 1);
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, p);
    return check_launch();
}

}  // namespace seld
