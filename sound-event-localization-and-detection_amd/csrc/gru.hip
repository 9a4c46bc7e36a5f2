// GRU recurrence (include/seld_hip.h, "GRU"): the sequential part of a torch.nn.GRU layer, every direction in one launch.
//
// One workgroup per (direction, tile of 16 batch columns); no workgroup talks to another, so there is no grid-wide
// barrier and no atomic.  W_hh (3H x H) stays in registers for the whole launch as A fragments of v_mfma_f32_16x16x4_f32:
// wave w owns hidden units 16w .. 16w+15 and their r, z, n row tiles (3 * Hp/4 registers per lane, 96 at Hp = 128), so the
// gate arithmetic of a unit never leaves its wave.  h (Hp x 16) is the B operand, double-buffered in LDS with one barrier
// per step; gx of the next step is loaded before the MFMA chain of this one.  The accumulator layout (column = lane & 15,
// rows 4 (lane >> 4) + i) gives every lane four consecutive hidden units of one batch column: that is the lane's slice of
// every global tensor, 16 bytes when H % 4 == 0.
//
// The backward kernel is the same machine with W_hh^T (H x 3H) resident: dgh (3Hp x 16) is the B operand.
//
// H that is no multiple of 16 runs zero-padded to Hp: a padded unit has zero weight rows and columns, zero bias, zero gx
// and zero h0, so r = z = 1/2, n = 0 and h stays exactly 0; it is never stored.  Columns past B compute on zeros and are
// never stored either.  A column's arithmetic does not depend on its neighbours: a sample gives the same bits alone and
// inside any batch, at any column.
#include <stdio.h>

#include "common.h"

namespace seld {

struct GruP {
    int dirs, B, T, H, vec;
    const float* gx;        // fwd: (dirs, B, T, 3H)
    const float* wpack;
    const float* h0;        // fwd: h0, bwd: dh_n (nullable)
    const float* dy;        // bwd
    float* y;               // fwd: y, bwd: unused
    float* hn;              // fwd: h_n, bwd: dh0 (nullable)
    float* saved;           // (5, dirs, B, T, H): r, z, n, W_hn h + b_hn, h_prev (fwd: nullable)
    float* dgx;             // bwd
    float* dgh;             // bwd
};

// the lane's four consecutive floats at p; `n` of them exist (0..4; with `vec` 0 or 4 and p 16-byte aligned)
__device__ __forceinline__ void ld4(const float* p, int n, int vec, float v[4]) {
    if (vec) {
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n) t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = i < n ? p[i] : 0.f;
    }
}
__device__ __forceinline__ void st4(float* p, int n, int vec, const float v[4]) {
    if (vec) {
        if (n) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < n) p[i] = v[i];
    }
}

// Both keep their relative accuracy near 0 (the 1 - 2 / (1 + exp(2x)) form of tanh cancels there).
__device__ __forceinline__ float gru_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float gru_tanh(float x) {
    const float ax = fabsf(x);
    // |x| < 1/4: the odd Taylor series through x^11, truncation below 1e-10 relative
    const float s = x * x;
    float p = -1382.0f / 155925.0f;
    p = fmaf(p, s, 62.0f / 2835.0f);
    p = fmaf(p, s, -17.0f / 315.0f);
    p = fmaf(p, s, 2.0f / 15.0f);
    p = fmaf(p, s, -1.0f / 3.0f);
    const float small = fmaf(x * s, p, x);
    const float e = __expf(-2.0f * ax);
    const float big = copysignf((1.0f - e) * __builtin_amdgcn_rcpf(1.0f + e), x);
    return ax < 0.25f ? small : big;
}

__host__ __device__ constexpr size_t gru_form_floats(int Hp) { return (size_t)3 * Hp * Hp; }

// wpack = [forward forms (dirs) | backward forms (dirs) | b_hh (dirs, 3, Hp)], zero where a unit is padding:
//   forward  (d, w, g, kc, lane) = W_d[g H + 16 w + (lane & 15)][4 kc + (lane >> 4)]      A[row = unit][k = input unit]
//   backward (d, w, g, kc, lane) = W_d[g H + 4 kc + (lane >> 4)][16 w + (lane & 15)]      A[row = input unit][k = gate row]
__global__ __launch_bounds__(256) void gru_pack_kernel(int dirs, int H, int Hp, const float* w0, const float* w1,
                                                       const float* b0, const float* b1, float* out) {
    const size_t form = gru_form_floats(Hp), nform = 2 * (size_t)dirs * form, total = nform + (size_t)dirs * 3 * Hp;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float v = 0.f;
    if (i < nform) {
        const int bwd = i >= (size_t)dirs * form;
        size_t r = i - (bwd ? (size_t)dirs * form : 0);
        const int d = (int)(r / form);
        r -= d * form;
        const int KC = Hp / 4;
        const int lane = (int)(r & 63), kc = (int)((r >> 6) % KC), g = (int)((r >> 6) / KC % 3), w = (int)((r >> 6) / KC / 3);
        const int a = 16 * w + (lane & 15), k = 4 * kc + (lane >> 4);
        const float* W = d ? w1 : w0;
        if (a < H && k < H) v = bwd ? W[((size_t)g * H + k) * H + a] : W[((size_t)g * H + a) * H + k];
    } else {
        const size_t r = i - nform;
        const int d = (int)(r / (3 * Hp)), g = (int)(r / Hp % 3), j = (int)(r % Hp);
        const float* b = d ? b1 : b0;
        if (b && j < H) v = b[g * H + j];
    }
    out[i] = v;
}

template <int NW>
__global__ __launch_bounds__(NW * 64) void gru_fwd_kernel(GruP p) {
    constexpr int HP = 16 * NW, KC = 4 * NW;
    __shared__ float hl[2][HP * 16];
    const int dir = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = lane & 15, q = lane >> 4, j0 = 16 * w + 4 * q;
    const int b = blockIdx.x * 16 + col, H = p.H, T = p.T;
    const int nv = b < p.B ? min(max(H - j0, 0), 4) : 0;        // this lane's live units
    const size_t bd = (size_t)dir * p.B + (nv ? b : 0);

    float a[3][KC];
    {
        const float* af = p.wpack + (size_t)dir * gru_form_floats(HP) + (size_t)w * 3 * KC * 64 + lane;
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) a[g][kc] = af[(g * KC + kc) * 64];
    }
    float bh[3][4];
    {
        const float* bp = p.wpack + 2 * (size_t)p.dirs * gru_form_floats(HP) + (size_t)dir * 3 * HP + j0;
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) bh[g][i] = bp[g * HP + i];
    }
    float h[4];
    ld4(p.h0 ? p.h0 + bd * H + j0 : nullptr, p.h0 ? nv : 0, p.vec, h);
#pragma unroll
    for (int i = 0; i < 4; ++i) hl[0][(j0 + i) * 16 + col] = h[i];
    __syncthreads();

    const float* gxp = p.gx + bd * T * 3 * H + j0;
    const size_t plane = (size_t)p.dirs * p.B * T * H;         // one saved tensor
    float gn[3][4];
    {
        const int t = dir ? T - 1 : 0;
#pragma unroll
        for (int g = 0; g < 3; ++g) ld4(gxp + (size_t)t * 3 * H + g * H, nv, p.vec, gn[g]);
    }
    int cur = 0;
    for (int s = 0; s < T; ++s) {
        const int t = dir ? T - 1 - s : s;
        float gc[3][4];
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) gc[g][i] = gn[g][i];
        if (s + 1 < T) {
            const int tn = dir ? t - 1 : t + 1;
#pragma unroll
            for (int g = 0; g < 3; ++g) ld4(gxp + (size_t)tn * 3 * H + g * H, nv, p.vec, gn[g]);
        }
        floatx4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        const float* hb = hl[cur] + q * 16 + col;               // B[k = 4 kc + q][col]
#pragma unroll
        for (int kc = 0; kc < KC; ++kc) {
            const float bv = hb[kc * 64];
#pragma unroll
            for (int g = 0; g < 3; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][kc], bv, acc[g], 0, 0, 0);
        }
        float r[4], z[4], n[4], qn[4], hnew[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            r[i] = gru_sigmoid(gc[0][i] + (acc[0][i] + bh[0][i]));
            z[i] = gru_sigmoid(gc[1][i] + (acc[1][i] + bh[1][i]));
            qn[i] = acc[2][i] + bh[2][i];
            n[i] = gru_tanh(fmaf(r[i], qn[i], gc[2][i]));
            hnew[i] = fmaf(z[i], h[i] - n[i], n[i]);            // (1 - z) n + z h
        }
        const size_t at = (bd * T + t) * H + j0;
        if (p.saved) {
            st4(p.saved + at, nv, p.vec, r);
            st4(p.saved + plane + at, nv, p.vec, z);
            st4(p.saved + 2 * plane + at, nv, p.vec, n);
            st4(p.saved + 3 * plane + at, nv, p.vec, qn);
            st4(p.saved + 4 * plane + at, nv, p.vec, h);
        }
        st4(p.y + ((size_t)(nv ? b : 0) * T + t) * p.dirs * H + (size_t)dir * H + j0, nv, p.vec, hnew);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            h[i] = hnew[i];
            hl[cur ^ 1][(j0 + i) * 16 + col] = hnew[i];
        }
        __syncthreads();
        cur ^= 1;
    }
    st4(p.hn + bd * H + j0, nv, p.vec, h);
}

template <int NW>
__global__ __launch_bounds__(NW * 64) void gru_bwd_kernel(GruP p) {
    constexpr int HP = 16 * NW, KC = 4 * NW;
    __shared__ float dl[2][3 * HP * 16];
    const int dir = blockIdx.y, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = lane & 15, q = lane >> 4, j0 = 16 * w + 4 * q;
    const int b = blockIdx.x * 16 + col, H = p.H, T = p.T;
    const int nv = b < p.B ? min(max(H - j0, 0), 4) : 0;
    const size_t bd = (size_t)dir * p.B + (nv ? b : 0);

    float a[3][KC];
    {
        const float* ab = p.wpack + (size_t)(p.dirs + dir) * gru_form_floats(HP) + (size_t)w * 3 * KC * 64 + lane;
#pragma unroll
        for (int g = 0; g < 3; ++g)
#pragma unroll
            for (int kc = 0; kc < KC; ++kc) a[g][kc] = ab[(g * KC + kc) * 64];
    }
    float dhc[4];                                               // dh carried from the later step
    ld4(p.h0 ? p.h0 + bd * H + j0 : nullptr, p.h0 ? nv : 0, p.vec, dhc);

    const size_t plane = (size_t)p.dirs * p.B * T * H;
    const float* dyp = p.dy + (size_t)(nv ? b : 0) * T * p.dirs * H + (size_t)dir * H + j0;
    float sn[6][4];                                             // r, z, n, W_hn h + b_hn, h_prev, dy of the next step
    {
        const int t = dir ? 0 : T - 1;
        const size_t at = (bd * T + t) * H + j0;
#pragma unroll
        for (int k = 0; k < 5; ++k) ld4(p.saved + k * plane + at, nv, p.vec, sn[k]);
        ld4(dyp + (size_t)t * p.dirs * H, nv, p.vec, sn[5]);
    }
    int cur = 0;
    for (int s = T - 1; s >= 0; --s) {
        const int t = dir ? T - 1 - s : s;
        float sc[6][4];
#pragma unroll
        for (int k = 0; k < 6; ++k)
#pragma unroll
            for (int i = 0; i < 4; ++i) sc[k][i] = sn[k][i];
        if (s > 0) {
            const int tn = dir ? t + 1 : t - 1;
            const size_t at = (bd * T + tn) * H + j0;
#pragma unroll
            for (int k = 0; k < 5; ++k) ld4(p.saved + k * plane + at, nv, p.vec, sn[k]);
            ld4(dyp + (size_t)tn * p.dirs * H, nv, p.vec, sn[5]);
        }
        float dh[4], dg[3][4], dn[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float r = sc[0][i], z = sc[1][i], n = sc[2][i], qn = sc[3][i], hp = sc[4][i];
            dh[i] = dhc[i] + sc[5][i];
            dn[i] = dh[i] * (1.0f - z) * fmaf(-n, n, 1.0f);     // through tanh
            dg[0][i] = dn[i] * qn * r * (1.0f - r);
            dg[1][i] = dh[i] * (hp - n) * z * (1.0f - z);
            dg[2][i] = dn[i] * r;                               // dgh's n part; dgx's is dn
        }
        const size_t at = (bd * T + t) * 3 * H + j0;
        st4(p.dgx + at, nv, p.vec, dg[0]);
        st4(p.dgx + at + H, nv, p.vec, dg[1]);
        st4(p.dgx + at + 2 * H, nv, p.vec, dn);
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            st4(p.dgh + at + g * H, nv, p.vec, dg[g]);
#pragma unroll
            for (int i = 0; i < 4; ++i) dl[cur][(g * HP + j0 + i) * 16 + col] = dg[g][i];
        }
        __syncthreads();
        floatx4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        const float* db = dl[cur] + q * 16 + col;               // B[k = g Hp + 4 kc + q][col]
#pragma unroll
        for (int kc = 0; kc < KC; ++kc)
#pragma unroll
            for (int g = 0; g < 3; ++g)
                acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[g][kc], db[g * HP * 16 + kc * 64], acc[g], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) dhc[i] = fmaf(dh[i], sc[1][i], (acc[0][i] + acc[1][i]) + acc[2][i]);
        cur ^= 1;
    }
    if (p.hn) st4(p.hn + bd * H + j0, nv, p.vec, dhc);
}

static int gru_args(int dirs, int64_t B, int64_t T, int H) {
    if (dirs < 1 || dirs > 2 || B <= 0 || T <= 0 || H <= 0) return SELD_EINVAL;
    if (H > SELD_GRU_MAX_HIDDEN) return SELD_EUNSUPPORTED;
    if (5 * dirs * B * T >= ((int64_t)1 << 31) / H) return SELD_EUNSUPPORTED;      // the saved tensors are the largest
    return SELD_OK;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

#define GRU_DISPATCH(kernel, nw, grid, st, p)                                                     \
    switch (nw) {                                                                                 \
        case 1: hipLaunchKernelGGL(kernel<1>, grid, dim3(64), 0, st, p); break;                   \
        case 2: hipLaunchKernelGGL(kernel<2>, grid, dim3(128), 0, st, p); break;                  \
        case 3: hipLaunchKernelGGL(kernel<3>, grid, dim3(192), 0, st, p); break;                  \
        case 4: hipLaunchKernelGGL(kernel<4>, grid, dim3(256), 0, st, p); break;                  \
        case 5: hipLaunchKernelGGL(kernel<5>, grid, dim3(320), 0, st, p); break;                  \
        case 6: hipLaunchKernelGGL(kernel<6>, grid, dim3(384), 0, st, p); break;                  \
        case 7: hipLaunchKernelGGL(kernel<7>, grid, dim3(448), 0, st, p); break;                  \
        default: hipLaunchKernelGGL(kernel<8>, grid, dim3(512), 0, st, p); break;                 \
    }

}  // namespace seld
using namespace seld;

extern "C" size_t seld_gru_pack_floats(int32_t dirs, int32_t H) {
    if (dirs < 1 || dirs > 2 || H <= 0 || H > SELD_GRU_MAX_HIDDEN) return 0;
    const int Hp = (H + 15) / 16 * 16;
    return (size_t)dirs * (2 * gru_form_floats(Hp) + 3 * Hp);
}

extern "C" int seld_gru_pack(int32_t dirs, int32_t H, const float* w_hh0, const float* w_hh1, const float* b_hh0,
                             const float* b_hh1, float* wpack, void* stream) {
    if (dirs < 1 || dirs > 2 || H <= 0 || !w_hh0 || (dirs == 2 && !w_hh1) || !wpack) return SELD_EINVAL;
    if (dirs == 2 && (b_hh0 == nullptr) != (b_hh1 == nullptr)) return SELD_EINVAL;
    if (H > SELD_GRU_MAX_HIDDEN) return SELD_EUNSUPPORTED;
    const size_t total = seld_gru_pack_floats(dirs, H);
    hipLaunchKernelGGL(gru_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dirs, H,
                       (H + 15) / 16 * 16, w_hh0, w_hh1, b_hh0, b_hh1, wpack);
    return check_launch();
}

extern "C" size_t seld_gru_saved_floats(int32_t dirs, int32_t B, int32_t T, int32_t H) {
    if (gru_args(dirs, B, T, H)) return 0;
    return (size_t)5 * dirs * B * T * H;
}

extern "C" int seld_gru_fwd(int32_t dirs, int32_t B, int32_t T, int32_t H, const float* gx, const float* wpack,
                            const float* h0, float* y, float* h_n, float* saved, size_t saved_floats, void* stream) {
    int rc = gru_args(dirs, B, T, H);
    if (rc) return rc;
    if (!gx || !wpack || !y || !h_n) return SELD_EINVAL;
    if (saved && saved_floats < seld_gru_saved_floats(dirs, B, T, H)) return SELD_EWORKSPACE;
    GruP p{};
    p.dirs = dirs; p.B = B; p.T = T; p.H = H;
    p.gx = gx; p.wpack = wpack; p.h0 = h0; p.y = y; p.hn = h_n; p.saved = saved;
    p.vec = H % 4 == 0 && aligned16(gx) && aligned16(y) && aligned16(h_n) && aligned16(h0) && aligned16(saved);
    const dim3 grid((B + 15) / 16, dirs);
    GRU_DISPATCH(gru_fwd_kernel, (H + 15) / 16, grid, (hipStream_t)stream, p);
    return check_launch();
}

extern "C" int seld_gru_bwd(int32_t dirs, int32_t B, int32_t T, int32_t H, const float* dy, const float* dh_n,
                            const float* wpack, const float* saved, size_t saved_floats, float* dgx, float* dgh,
                            float* dh0, void* stream) {
    int rc = gru_args(dirs, B, T, H);
    if (rc) return rc;
    if (!dy || !wpack || !saved || !dgx || !dgh) return SELD_EINVAL;
    if (saved_floats < seld_gru_saved_floats(dirs, B, T, H)) return SELD_EWORKSPACE;
    GruP p{};
    p.dirs = dirs; p.B = B; p.T = T; p.H = H;
    p.dy = dy; p.wpack = wpack; p.h0 = dh_n; p.hn = dh0; p.saved = const_cast<float*>(saved); p.dgx = dgx; p.dgh = dgh;
    p.vec = H % 4 == 0 && aligned16(dy) && aligned16(dh_n) && aligned16(saved) && aligned16(dgx) && aligned16(dgh) &&
            aligned16(dh0);
    const dim3 grid((B + 15) / 16, dirs);
    GRU_DISPATCH(gru_bwd_kernel, (H + 15) / 16, grid, (hipStream_t)stream, p);
    return check_launch();
}

extern "C" int seld_gru_kernel_label(int32_t op, int32_t H, char* buf, int32_t buflen) {
    if ((op != SELD_GRU_FWD && op != SELD_GRU_BWD) || !buf || buflen < 32 || H <= 0) return SELD_EINVAL;
    if (H > SELD_GRU_MAX_HIDDEN) return SELD_EUNSUPPORTED;
    snprintf(buf, buflen, "gru_%s_kernel<%d>", op == SELD_GRU_FWD ? "fwd" : "bwd", (H + 15) / 16);
    return SELD_OK;
}
