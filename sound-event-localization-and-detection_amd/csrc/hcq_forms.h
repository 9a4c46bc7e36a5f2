// The 8-multiplication Hamilton product, written down once for every fast-product kernel (hcq_conv.hip, hcq_wgrad.hip,
// hcq_wgrad_grp.hip), and the two memory helpers those kernels share.
//
// c = a (x) b (a on the left) is a bilinear map of rank 8: with the sums of two components
//
//     P0 = (a3 + a1)(b1 + b2)   P1 = (a0 - a2)(b0 + b3)   P2 = (a0 + a2)(b0 - b3)   P3 = (a3 - a1)(b1 - b2)
//     P4 = (a3 - a2)(b2 - b3)   P5 = (a1 + a0)(b1 + b0)   P6 = (a0 - a1)(b2 + b3)   P7 = (a3 + a2)(b1 - b0)
//
//     c0 = (-P0 + P1 + P2 + P3)/2 + P4      c1 = (-P0 - P1 - P2 + P3)/2 + P5
//     c2 = ( P0 - P1 + P2 + P3)/2 + P6      c3 = ( P0 + P1 - P2 + P3)/2 - P7
//
// P_m = F_m(a) G_m(b).  The tables below are these lines; the static_assert behind them holds them to quat_comp /
// quat_sign of common.h, which define the product for the rest of the library.
#pragma once
#include "common.h"

namespace seld {

struct HcqForm { int c1, c2, s1, s2; };      // s1 * v[c1] + s2 * v[c2]
constexpr HcqForm HCQ_F[8] = {{3, 1, 1, 1}, {0, 2, 1, -1}, {0, 2, 1, 1}, {3, 1, 1, -1},
                              {3, 2, 1, -1}, {1, 0, 1, 1}, {0, 1, 1, -1}, {3, 2, 1, 1}};
constexpr HcqForm HCQ_G[8] = {{1, 2, 1, 1}, {0, 3, 1, 1}, {0, 3, 1, -1}, {1, 2, 1, -1},
                              {2, 3, 1, -1}, {1, 0, 1, 1}, {2, 3, 1, 1}, {1, 0, 1, -1}};
constexpr int HCQ_R2[4][8] = {{-1, 1, 1, 1, 2, 0, 0, 0},      // 2 c_q = sum_m R2[q][m] P_m
                              {-1, -1, -1, 1, 0, 2, 0, 0},
                              {1, -1, 1, 1, 0, 0, 2, 0},
                              {1, 1, -1, 1, 0, 0, 0, -2}};

// G_m(conj x), F_m(conj a): the conjugate flips the sign of components 1 to 3
constexpr HcqForm hcq_conj(HcqForm f) { return {f.c1, f.c2, f.c1 ? -f.s1 : f.s1, f.c2 ? -f.s2 : f.s2}; }

// A form in the shape the grouped weight gradient evaluates: s1 * (x[c1] + t * x[c2]), the positive term first where
// there is one, so that s1 (applied once, by the fold) is negative only for the forms whose two terms both are.
struct HcqSplit { int c1, c2, s1, t; };
constexpr HcqSplit hcq_split(HcqForm f) {
    return (f.s1 < 0 && f.s2 > 0) ? HcqSplit{f.c2, f.c1, 1, -1} : HcqSplit{f.c1, f.c2, f.s1, f.s1 * f.s2};
}

// The value of a form.  Each sign pattern keeps ONE rounding: a + b, a - b, b - a, -(a + b).
__host__ __device__ constexpr float hcq_eval(HcqForm f, const float v[4]) {
    return f.s1 > 0 ? (f.s2 > 0 ? v[f.c1] + v[f.c2] : v[f.c1] - v[f.c2])
                    : (f.s2 > 0 ? v[f.c2] - v[f.c1] : -(v[f.c1] + v[f.c2]));
}
template <int M> __host__ __device__ constexpr float hcq_f(const float a[4]) { constexpr HcqForm f = HCQ_F[M]; return hcq_eval(f, a); }
template <int M> __host__ __device__ constexpr float hcq_g(const float b[4]) { constexpr HcqForm f = HCQ_G[M]; return hcq_eval(f, b); }
template <int M> __host__ __device__ constexpr float hcq_gc(const float x[4]) { constexpr HcqForm f = hcq_conj(HCQ_G[M]); return hcq_eval(f, x); }

// The 8 -> 4 recombination.  The association is part of the result's bits: halves of P0..P3 first, then
// (h3 -+ h0) +- (h1 +- h2), then the single form.
struct HcqQuat { float c[4]; };
__host__ __device__ constexpr HcqQuat hcq_recombine(float P0, float P1, float P2, float P3, float P4, float P5, float P6, float P7) {
    const float h0 = 0.5f * P0, h1 = 0.5f * P1, h2 = 0.5f * P2, h3 = 0.5f * P3;
    return {{(h3 - h0) + (h1 + h2) + P4, (h3 - h0) - (h1 + h2) + P5, (h3 + h0) + (h2 - h1) + P6, (h3 + h0) + (h1 - h2) - P7}};
}

// the same on the four elements of an accumulator fragment: c[q][r] from P[m][r]
__device__ __forceinline__ void hcq_recombine4(const floatx4 P[8], floatx4 c[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const HcqQuat v = hcq_recombine(P[0][r], P[1][r], P[2][r], P[3][r], P[4][r], P[5][r], P[6][r], P[7][r]);
#pragma unroll
        for (int q = 0; q < 4; ++q) c[q][r] = v.c[q];
    }
}

// ---- the proof ------------------------------------------------------------------------------------------------------
// For every pair of basis elements (e_i on the left, e_j on the right) and every output component q:
//     sum_m R2[q][m] F_m(e_i) G_m(e_j)  =  2 quat_sign(q, j)  if quat_comp(q, j) == i,  else 0
// with F_m, G_m evaluated by the functions the kernels call, and hcq_recombine is R2 / 2 on the unit vectors of P.
constexpr bool hcq_forms_are_the_hamilton_product() {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
            a[i] = 1.f;
            b[j] = 1.f;
            const float P[8] = {hcq_f<0>(a) * hcq_g<0>(b), hcq_f<1>(a) * hcq_g<1>(b), hcq_f<2>(a) * hcq_g<2>(b), hcq_f<3>(a) * hcq_g<3>(b),
                                hcq_f<4>(a) * hcq_g<4>(b), hcq_f<5>(a) * hcq_g<5>(b), hcq_f<6>(a) * hcq_g<6>(b), hcq_f<7>(a) * hcq_g<7>(b)};
            const HcqQuat c = hcq_recombine(P[0], P[1], P[2], P[3], P[4], P[5], P[6], P[7]);
            for (int q = 0; q < 4; ++q) {
                float s2 = 0.f;
                for (int m = 0; m < 8; ++m) s2 += (float)HCQ_R2[q][m] * P[m];
                const float want = quat_comp(q, j) == i ? 2.f * quat_sign(q, j) : 0.f;
                if (s2 != want || 2.f * c.c[q] != want) return false;
            }
        }
    return true;
}
static_assert(hcq_forms_are_the_hamilton_product(), "F_m, G_m, R2 and hcq_recombine must be the Hamilton product of common.h");

// ---- device helpers -------------------------------------------------------------------------------------------------
__device__ __forceinline__ void hcq_xforms(const float b[4], float g[8]) {
    g[0] = hcq_g<0>(b); g[1] = hcq_g<1>(b); g[2] = hcq_g<2>(b); g[3] = hcq_g<3>(b);
    g[4] = hcq_g<4>(b); g[5] = hcq_g<5>(b); g[6] = hcq_g<6>(b); g[7] = hcq_g<7>(b);
}
__device__ __forceinline__ void hcq_fforms(const float a[4], float f[8]) {
    f[0] = hcq_f<0>(a); f[1] = hcq_f<1>(a); f[2] = hcq_f<2>(a); f[3] = hcq_f<3>(a);
    f[4] = hcq_f<4>(a); f[5] = hcq_f<5>(a); f[6] = hcq_f<6>(a); f[7] = hcq_f<7>(a);
}
__device__ __forceinline__ void hcq_gforms_conj(const float x[4], float g[8]) {
    g[0] = hcq_gc<0>(x); g[1] = hcq_gc<1>(x); g[2] = hcq_gc<2>(x); g[3] = hcq_gc<3>(x);
    g[4] = hcq_gc<4>(x); g[5] = hcq_gc<5>(x); g[6] = hcq_gc<6>(x); g[7] = hcq_gc<7>(x);
}
// F_m(a) for a form index known only at run time (one thread per packed float)
__device__ __forceinline__ float hcq_form_f(int m, const float a[4]) {
    switch (m) {
        case 0: return hcq_f<0>(a);
        case 1: return hcq_f<1>(a);
        case 2: return hcq_f<2>(a);
        case 3: return hcq_f<3>(a);
        case 4: return hcq_f<4>(a);
        case 5: return hcq_f<5>(a);
        case 6: return hcq_f<6>(a);
        default: return hcq_f<7>(a);
    }
}

typedef int int4h __attribute__((ext_vector_type(4)));

// One 16-byte-per-lane LDS-DMA: LDS[lds_addr + 16 * lane ..] <- buffer[soff + voff ..] (zeros when voff is out of range);
// lanes that are switched off write nothing.  Inline asm: the kernels count these loads themselves (the compiler's
// waitcnt pass would put vmcnt(0) in front of every LDS read that follows).  M0 is saved and restored in the statement.
__device__ __forceinline__ void hcq_dma16(unsigned lds_addr, unsigned voff, int4h rsrc, unsigned soff) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_addr), "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}
__device__ __forceinline__ void hcq_dma16(unsigned lds_addr, unsigned voff, int4h rsrc) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_addr), "v"(voff), "s"(rsrc) : "memory");
}
// raw buffer resource over [base, base + bytes)
__device__ __forceinline__ int4h hcq_rsrc(const float* base, unsigned bytes) {
    const unsigned long long a = (unsigned long long)base;
    return (int4h){(int)(unsigned)a, (int)((unsigned)(a >> 32) & 0xFFFFu), (int)bytes, 0x00020000};
}

}  // namespace seld
