// STFT magnitude / phase for every segment length 2 <= N <= 4096 that the power-of-two kernels of stft.hip do not take
// (utility_functions.py:129-155; same boundary, padding, window and output layout as stft_kernel).
//
// One workgroup transforms FT consecutive frames of one channel.  Two real frames go in as the real and imaginary part
// of one complex signal (FT / 2 transforms side by side in LDS) and are separated in the epilogue,
// A[k] = (Z[k] + conj Z[N-k]) / 2, B[k] = (Z[k] - conj Z[N-k]) / 2i -- for odd N as for even N.
//
//   7-smooth N (2^a 3^b 5^c 7^d): a mixed-radix Stockham FFT of length N in LDS, radices 8/4/2, 7, 5, 3, twiddles from
//     an LDS table W_N^t built with sincospif.
//   any other N: Bluestein / chirp-z.  With b[n] = exp(i pi n^2 / N), X[k] = conj(b[k]) sum_n (x[n] conj b[n]) b[k-n]: a
//     circular convolution of length M = 2^ceil(log2(2N - 1)) <= 8192, done as FFT_M, a pointwise product with the
//     chirp's spectrum and a second forward FFT_M of the conjugate (IFFT(Y) = conj(FFT(conj Y)) / M).  The chirp, its
//     spectrum (already divided by M) live in the caller's workspace, filled once per call by stft_chirp_kernel; the
//     chirp angle pi (n^2 mod 2N) / N is reduced in integers before sincospif.  Twiddles W_M^t = W_M^(64 hi) W_M^lo from
//     two short LDS tables (a full one does not fit beside two 8192-point buffers).
//
// The epilogue reads |Z| / angle(Z) straight from the transform buffers in [bin][frame] order and stores with the frame
// index fastest (the output's contiguous axis).  No atomics: results are run-to-run identical.
#include "common.h"

namespace seld {
namespace {

__device__ __forceinline__ float2 c_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 c_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 c_mul(float2 a, float2 b) {
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 c_mul_mi(float2 a) { return make_float2(a.y, -a.x); }     // a * (-i)
__device__ __forceinline__ float2 c_conj(float2 a) { return make_float2(a.x, -a.y); }

// cos / sin (2 pi m / R) for the odd radices
__device__ __forceinline__ constexpr float odd_cos(int R, int m) {
    return R == 3 ? (m == 0 ? 1.f : -0.5f)
         : R == 5 ? (m == 0 ? 1.f : (m == 1 || m == 4) ? 0.30901699437494745f : -0.80901699437494745f)
         : (m == 0 ? 1.f : (m == 1 || m == 6) ? 0.62348980185873353f : (m == 2 || m == 5) ? -0.22252093395631440f
                                                                                       : -0.90096886790241913f);
}
__device__ __forceinline__ constexpr float odd_sin(int R, int m) {
    return R == 3 ? (m == 0 ? 0.f : m == 1 ? 0.86602540378443865f : -0.86602540378443865f)
         : R == 5 ? (m == 0 ? 0.f : m == 1 ? 0.95105651629515357f : m == 2 ? 0.58778525229247313f
                     : m == 3 ? -0.58778525229247313f : -0.95105651629515357f)
         : (m == 0 ? 0.f : m == 1 ? 0.78183148246802981f : m == 2 ? 0.97492791218182361f : m == 3 ? 0.43388373911755812f
            : m == 4 ? -0.43388373911755812f : m == 5 ? -0.97492791218182361f : -0.78183148246802981f);
}

// forward R-point DFT in place (exp(-2 pi i r q / R)), outputs in natural order
template <int R> __device__ __forceinline__ void dft(float2 (&v)[R]);
template <> __device__ __forceinline__ void dft<2>(float2 (&v)[2]) {
    const float2 a = v[0], b = v[1];
    v[0] = c_add(a, b); v[1] = c_sub(a, b);
}
template <> __device__ __forceinline__ void dft<4>(float2 (&v)[4]) {
    const float2 c0 = c_add(v[0], v[2]), c2 = c_sub(v[0], v[2]), c1 = c_add(v[1], v[3]), c3 = c_mul_mi(c_sub(v[1], v[3]));
    v[0] = c_add(c0, c1); v[2] = c_sub(c0, c1); v[1] = c_add(c2, c3); v[3] = c_sub(c2, c3);
}
template <> __device__ __forceinline__ void dft<8>(float2 (&v)[8]) {
    constexpr float H = 0.70710678118654752f;
    float2 a0 = c_add(v[0], v[4]), a4 = c_sub(v[0], v[4]);
    float2 a1 = c_add(v[1], v[5]), a5 = c_sub(v[1], v[5]);
    float2 a2 = c_add(v[2], v[6]), a6 = c_sub(v[2], v[6]);
    float2 a3 = c_add(v[3], v[7]), a7 = c_sub(v[3], v[7]);
    a5 = make_float2(H * (a5.x + a5.y), H * (a5.y - a5.x));          // * (1 - i) / sqrt 2
    a6 = c_mul_mi(a6);
    a7 = make_float2(H * (a7.y - a7.x), -H * (a7.x + a7.y));         // * (-1 - i) / sqrt 2
    {
        const float2 c0 = c_add(a0, a2), c2 = c_sub(a0, a2), c1 = c_add(a1, a3), c3 = c_mul_mi(c_sub(a1, a3));
        v[0] = c_add(c0, c1); v[4] = c_sub(c0, c1); v[2] = c_add(c2, c3); v[6] = c_sub(c2, c3);
    }
    {
        const float2 c0 = c_add(a4, a6), c2 = c_sub(a4, a6), c1 = c_add(a5, a7), c3 = c_mul_mi(c_sub(a5, a7));
        v[1] = c_add(c0, c1); v[5] = c_sub(c0, c1); v[3] = c_add(c2, c3); v[7] = c_sub(c2, c3);
    }
}
// odd R: X[q] = v0 + sum_{r <= R/2} (s_r cos - i d_r sin)(2 pi r q / R), X[R-q] its mirror, s_r / d_r = v[r] +- v[R-r]
template <int R> __device__ __forceinline__ void dft_odd(float2 (&v)[R]) {
    constexpr int H = R / 2;
    float2 s[H + 1], d[H + 1];
    float2 y0 = v[0];
#pragma unroll
    for (int r = 1; r <= H; ++r) {
        s[r] = c_add(v[r], v[R - r]);
        d[r] = c_sub(v[r], v[R - r]);
        y0 = c_add(y0, s[r]);
    }
#pragma unroll
    for (int q = 1; q <= H; ++q) {
        float2 a = v[0], b = make_float2(0.f, 0.f);
#pragma unroll
        for (int r = 1; r <= H; ++r) {
            const float cs = odd_cos(R, (r * q) % R), sn = odd_sin(R, (r * q) % R);
            a.x += s[r].x * cs; a.y += s[r].y * cs;
            b.x += d[r].x * sn; b.y += d[r].y * sn;
        }
        v[q] = make_float2(a.x + b.y, a.y - b.x);           // a - i b
        v[R - q] = make_float2(a.x - b.y, a.y + b.x);       // a + i b
    }
    v[0] = y0;
}
template <> __device__ __forceinline__ void dft<3>(float2 (&v)[3]) { dft_odd<3>(v); }
template <> __device__ __forceinline__ void dft<5>(float2 (&v)[5]) { dft_odd<5>(v); }
template <> __device__ __forceinline__ void dft<7>(float2 (&v)[7]) { dft_odd<7>(v); }

// Twiddle W_P^i from a full table (LDS) or as W_P^(64 (i / 64)) * W_P^(i mod 64) from two short LDS tables (P / 64 + 64
// entries: the Bluestein lengths, whose full table does not fit beside two buffers of 8192 points)
struct TwFull {
    const float2* t;
    __device__ __forceinline__ float2 operator()(int i) const { return t[i]; }
};
struct TwSplit {
    const float2* hi;
    const float2* lo;
    __device__ __forceinline__ float2 operator()(int i) const { return c_mul(hi[i >> 6], lo[i & 63]); }
};
__device__ __forceinline__ void tw_split_build(float2* lo, float2* hi, int P, int tid) {
    for (int j = tid; j < 64 + ((P + 63) >> 6); j += 256) {
        const int e = j < 64 ? j : 64 * (j - 64);
        float sn, cs;
        sincospif(-2.0f * (float)e / (float)P, &sn, &cs);
        (j < 64 ? lo[j] : hi[j - 64]) = make_float2(cs, sn);
    }
}

// One radix-R Stockham pass over `ntr` transforms of length P (transform t at t * ts): sub-transforms of length Ns are
// merged into length Ns * R.  Butterfly j reads src[j + r P / R], twiddles by W_{Ns R}^{r k} (k = j mod Ns) = tw[r k P /
// (Ns R)] and writes dst[(j - k) R + k + r Ns]; after the last pass the transform is in natural order.
template <int R, class Tw>
__device__ __forceinline__ void fft_pass(const float2* __restrict__ src, float2* __restrict__ dst, int P, int Ns, int ntr,
                                         int ts, Tw tw, int tid) {
    const int Q = P / R;
    const int tstep = P / (Ns * R);
    for (int i = tid; i < ntr * Q; i += 256) {
        const int t = i / Q, j = i - t * Q;
        const int k = j % Ns;
        const float2* s = src + t * ts + j;
        float2 v[R];
#pragma unroll
        for (int r = 0; r < R; ++r) v[r] = s[r * Q];
        if (Ns > 1) {
#pragma unroll
            for (int r = 1; r < R; ++r) v[r] = c_mul(v[r], tw(r * k * tstep));
        }
        dft<R>(v);
        float2* d = dst + t * ts + (j - k) * R + k;
#pragma unroll
        for (int r = 0; r < R; ++r) d[r * Ns] = v[r];
    }
}

// Every pass of the plan (radices packed 4 bits each, first pass lowest); returns the buffer that holds the result.
template <class Tw>
__device__ __forceinline__ float2* fft_lds(float2* a, float2* b, int P, unsigned long long radices, int npass, int ntr,
                                           int ts, Tw tw, int tid) {
    int Ns = 1;
    for (int p = 0; p < npass; ++p) {
        const int R = (int)((radices >> (4 * p)) & 15u);
        switch (R) {
            case 8: fft_pass<8>(a, b, P, Ns, ntr, ts, tw, tid); break;
            case 4: fft_pass<4>(a, b, P, Ns, ntr, ts, tw, tid); break;
            case 2: fft_pass<2>(a, b, P, Ns, ntr, ts, tw, tid); break;
            case 3: fft_pass<3>(a, b, P, Ns, ntr, ts, tw, tid); break;
            case 5: fft_pass<5>(a, b, P, Ns, ntr, ts, tw, tid); break;
            default: fft_pass<7>(a, b, P, Ns, ntr, ts, tw, tid); break;
        }
        __syncthreads();
        float2* t = a; a = b; b = t;
        Ns *= R;
    }
    return a;
}

}  // namespace

// The Bluestein tables of one call, one workgroup: chirp[n] = exp(i pi n^2 / N) and spec = FFT_M(chirp extended
// circularly: B[j] = chirp[j], B[M - j] = chirp[j], 0 < j < N) / M.  LDS: 2 M + 64 + M / 64 float2.
__global__ __launch_bounds__(256) void stft_chirp_kernel(int N, int M, unsigned long long radices, int npass,
                                                         float2* __restrict__ chirp, float2* __restrict__ spec) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float2* buf0 = reinterpret_cast<float2*>(smem);
    float2* buf1 = buf0 + M;
    float2* twlo = buf1 + M;
    const int tid = threadIdx.x;
    tw_split_build(twlo, twlo + 64, M, tid);
    for (int j = tid; j < M; j += 256) {
        float sn, cs;
        const int n = j < N ? j : (j > M - N ? M - j : -1);
        float2 b = make_float2(0.f, 0.f);
        if (n >= 0) {
            const int n2 = (int)(((long long)n * n) % (2LL * N));      // exact: the angle's period is 2N in n^2
            sincospif((float)n2 / (float)N, &sn, &cs);
            b = make_float2(cs, sn);
            if (j < N) chirp[j] = b;
        }
        buf0[j] = b;
    }
    __syncthreads();
    const float2* res = fft_lds(buf0, buf1, M, radices, npass, 1, M, TwSplit{twlo + 64, twlo}, tid);
    const float inv_m = 1.0f / (float)M;                                 // exact: M is a power of two
    for (int j = tid; j < M; j += 256) spec[j] = make_float2(res[j].x * inv_m, res[j].y * inv_m);
}

// output_phase: 0 = |Z|, 1 = |Z| and angle(Z), kStftComplex = Re Z and Im Z in their places: CPLX, an instantiation of
// its own, so that the other two values run the code they always ran.
// bin0: first bin kept (1 = DC dropped); window_g (nullable): N window values already divided by their sum, null =
// periodic Hamming.  P: FFT length (N, or M for BLUE); ntr transforms of 2 frames each, transform t at t * ts in both
// LDS buffers.  BLUE: chirp / spec from stft_chirp_kernel.  Twiddles: the W_N table in LDS, or (BLUE) the two short
// tables of TwSplit.
template <bool BLUE, bool CPLX>
__global__ __launch_bounds__(256) void stft_any_kernel(const float* __restrict__ x, int C, int L, int N, int hop,
                                                       int frames_out, int output_phase, int bin0,
                                                       const float* __restrict__ window_g, int P,
                                                       unsigned long long radices, int npass, int ntr, int ts,
                                                       const float2* __restrict__ chirp, const float2* __restrict__ spec,
                                                       float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float2* buf0 = reinterpret_cast<float2*>(smem);                 // ntr * ts
    float2* buf1 = buf0 + ntr * ts;                                 // ntr * ts
    float2* twl = buf1 + ntr * ts;                                  // P, or (BLUE) 64 + ceil(P / 64)
    float* win = reinterpret_cast<float*>(twl + (BLUE ? 64 + ((P + 63) >> 6) : P));   // N
    const int tid = threadIdx.x;
    const int c = blockIdx.y;
    const int FT = 2 * ntr;
    const int m0 = blockIdx.x * FT;
    const int half = N >> 1;
    const float inv_wsum = 1.0f / (0.54f * (float)N);

    if constexpr (BLUE) {
        tw_split_build(twl, twl + 64, P, tid);
    } else {
        for (int j = tid; j < P; j += 256) {
            float sn, cs;
            sincospif(-2.0f * (float)j / (float)P, &sn, &cs);
            twl[j] = make_float2(cs, sn);
        }
    }
    for (int n = tid; n < N; n += 256)
        win[n] = window_g ? window_g[n] : (0.54f - 0.46f * cospif(2.0f * (float)n / (float)N)) * inv_wsum;
    __syncthreads();

    const float* xc = x + (size_t)c * L;
    for (int i = tid; i < ntr * P; i += 256) {
        const int t = i / P, n = i - t * P;
        const int m = m0 + 2 * t;
        float2 v = make_float2(0.f, 0.f);
        if (n < N) {
            const long long ia = (long long)m * hop - half + n, ib = ia + hop;
            const float w = win[n];
            v.x = (m < frames_out && ia >= 0 && ia < L) ? xc[ia] * w : 0.f;
            v.y = (m + 1 < frames_out && ib >= 0 && ib < L) ? xc[ib] * w : 0.f;
            if constexpr (BLUE) v = c_mul(v, c_conj(chirp[n]));
        }
        buf0[t * ts + n] = v;
    }
    __syncthreads();
    const auto tw = [&] {
        if constexpr (BLUE) return TwSplit{twl + 64, twl};
        else return TwFull{twl};
    }();
    float2* res = fft_lds(buf0, buf1, P, radices, npass, ntr, ts, tw, tid);
    if constexpr (BLUE) {
        // conj(Y * spec): the second forward transform of it is conj(M * IFFT(Y * spec)) = conj of the convolution
        for (int i = tid; i < ntr * P; i += 256) {
            const int t = i / P, j = i - t * P;
            res[t * ts + j] = c_conj(c_mul(res[t * ts + j], spec[j]));
        }
        __syncthreads();
        res = fft_lds(res, res == buf0 ? buf1 : buf0, P, radices, npass, ntr, ts, tw, tid);
    }

    // bins bin0 .. N/2 of both frames of every transform, frame index fastest in the stores
    const int nbins = half + 1 - bin0;
    const int nf = (frames_out - m0) < FT ? (frames_out - m0) : FT;
    const int lft = 31 - __builtin_clz(FT);
    for (int e = tid; e < nbins * FT; e += 256) {
        const int b = e >> lft, f = e & (FT - 1);
        if (f >= nf) continue;
        const int k = b + bin0, km = k == 0 ? 0 : N - k;
        const float2* r = res + (f >> 1) * ts;
        float2 z = r[k], y = r[km];
        if constexpr (BLUE) {                                        // X[k] = conj(b[k]) conj(conv[k]) = conj(b[k] conv'[k])
            z = c_conj(c_mul(z, chirp[k]));
            y = c_conj(c_mul(y, chirp[km]));
        }
        float re, im;
        if ((f & 1) == 0) { re = 0.5f * (z.x + y.x); im = 0.5f * (z.y - y.y); }
        else { re = 0.5f * (z.y + y.y); im = -0.5f * (z.x - y.x); }
        if constexpr (CPLX) {
            out[((size_t)c * nbins + b) * frames_out + m0 + f] = re;
            out[((size_t)(C + c) * nbins + b) * frames_out + m0 + f] = im;
        } else {
            out[((size_t)c * nbins + b) * frames_out + m0 + f] = sqrtf(re * re + im * im);
            if (output_phase) out[((size_t)(C + c) * nbins + b) * frames_out + m0 + f] = atan2f(im, re);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
namespace {

constexpr size_t kLdsMax = 160 * 1024;       // LDS per CU
// frames per workgroup are halved down to this: two workgroups per CU.  A 160 KB target (more frames per workgroup,
// one workgroup per CU) measured 1.5-1.6x slower at N = 882 ... 1764 and 997, no faster at 2048 / 4096 / 4095.
constexpr size_t kLdsTarget = 80 * 1024;
constexpr size_t kLdsDefault = 64 * 1024;    // above this the launch needs hipFuncAttributeMaxDynamicSharedMemorySize

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

bool smooth7(int n) {
    for (int p : {2, 3, 5, 7})
        while (n % p == 0) n /= p;
    return n == 1;
}

// radices of P, 4 bits each, first pass in the lowest bits: 8s, then a 4 or 2, then 7s, 5s and 3s
int make_plan(int P, unsigned long long* radices) {
    int np = 0;
    unsigned long long code = 0;
    auto push = [&](int r) { code |= (unsigned long long)r << (4 * np); ++np; };
    while (P % 8 == 0) { push(8); P /= 8; }
    if (P % 4 == 0) { push(4); P /= 4; }
    if (P % 2 == 0) { push(2); P /= 2; }
    for (int r : {7, 5, 3})
        while (P % r == 0) { push(r); P /= r; }
    *radices = code;
    return np;
}

struct AnyCfg {
    bool blue;
    int P, ts, ntr, npass;
    unsigned long long radices;
    size_t smem, smem_chirp, ws;
    size_t off_chirp;
};

size_t tw_entries(bool blue, int P) { return blue ? 64 + (size_t)((P + 63) >> 6) : (size_t)P; }

size_t any_smem(bool blue, int N, int P, int ntr, int ts) {
    return sizeof(float2) * ((size_t)2 * ntr * ts + tw_entries(blue, P)) + sizeof(float) * (size_t)N;
}

AnyCfg any_config(int N) {
    AnyCfg g{};
    g.blue = !smooth7(N);
    g.P = N;
    if (g.blue) {
        g.P = 1;
        while (g.P < 2 * N - 1) g.P <<= 1;
    }
    g.ts = g.P + 1;                            // one float2 between transforms: the epilogue's frame-fastest reads spread banks
    g.npass = make_plan(g.P, &g.radices);
    g.ntr = 8;
    while (g.ntr > 1 && any_smem(g.blue, N, g.P, g.ntr, g.ts) > kLdsTarget) g.ntr >>= 1;
    g.smem = any_smem(g.blue, N, g.P, g.ntr, g.ts);
    if (g.blue) {
        g.smem_chirp = sizeof(float2) * ((size_t)2 * g.P + tw_entries(true, g.P));
        g.off_chirp = align256(sizeof(float2) * (size_t)g.P);          // spec at 0
        g.ws = g.off_chirp + align256(sizeof(float2) * (size_t)N);
    }
    return g;
}

int set_lds(const void* kern, size_t smem) {
    if (smem > kLdsDefault &&
        hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) != hipSuccess)
        return SELD_ELAUNCH;
    return SELD_OK;
}

}  // namespace

// Workspace of the general path (0 for the 7-smooth lengths).
size_t stft_any_workspace(int N) { return any_config(N).ws; }

// The general path for 2 <= N <= 4096; arguments validated by the caller (stft.hip).
int stft_any_launch(const float* x, int C, int L, int N, int hop, int frames, int output_phase, int bin0,
                    const float* window, float* out, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    const AnyCfg g = any_config(N);
    if (g.smem > kLdsMax || g.smem_chirp > kLdsMax) return SELD_EUNSUPPORTED;
    if (g.ws > 0 && (!workspace || workspace_bytes < g.ws)) return SELD_EWORKSPACE;
    char* ws = static_cast<char*>(workspace);
    float2* spec = g.blue ? reinterpret_cast<float2*>(ws) : nullptr;
    float2* chirp = g.blue ? reinterpret_cast<float2*>(ws + g.off_chirp) : nullptr;
    const dim3 grid((frames + 2 * g.ntr - 1) / (2 * g.ntr), C);
    const bool cplx = output_phase == kStftComplex;
    if (g.blue) {
        const auto kernel = cplx ? stft_any_kernel<true, true> : stft_any_kernel<true, false>;
        int rc = set_lds((const void*)stft_chirp_kernel, g.smem_chirp);
        if (rc == SELD_OK) rc = set_lds((const void*)kernel, g.smem);
        if (rc != SELD_OK) return rc;
        hipLaunchKernelGGL(stft_chirp_kernel, dim3(1), dim3(256), g.smem_chirp, stream, N, g.P, g.radices, g.npass, chirp,
                           spec);
        rc = check_launch();
        if (rc != SELD_OK) return rc;
        hipLaunchKernelGGL(kernel, grid, dim3(256), g.smem, stream, x, C, L, N, hop, frames, output_phase,
                           bin0, window, g.P, g.radices, g.npass, g.ntr, g.ts, chirp, spec, out);
        return check_launch();
    }
    const auto kernel = cplx ? stft_any_kernel<false, true> : stft_any_kernel<false, false>;
    const int rc = set_lds((const void*)kernel, g.smem);
    if (rc != SELD_OK) return rc;
    hipLaunchKernelGGL(kernel, grid, dim3(256), g.smem, stream, x, C, L, N, hop, frames, output_phase,
                       bin0, window, g.P, g.radices, g.npass, g.ntr, g.ts, chirp, spec, out);
    return check_launch();
}

}  // namespace seld
