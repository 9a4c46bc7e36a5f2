// Shared declarations of the hypercomplex convolution kernels (hc_conv_fwd.hip, hc_wgrad.hip).
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include "common.h"
#include "env.h"

namespace seld {

enum { MODE_FWD = 0, MODE_DGRAD = 1 };

struct ConvP {
    int algebra, mode;
    int Csrc, Cdst;            // channels of the streamed operand / of the result
    int srcH, srcW, dstH, dstW;
    int KH, KW;
    int SMh, OFFh, KDh, SDh;   // src index = d*SM + OFF + k*KD, then (if SD > 1) must divide by SD
    int SMw, OFFw, KDw, SDw;
    int Ktot;                  // Csrc * KH * KW
    int OA, IA;                // Cout/A, Cin/A of the convolution
    int srcS, dstS;
    long long Ptot;            // N * dstS
    long long src_elems;       // N * Csrc * srcS
    int wt;                    // dgrad: component tensors are transposed to [c][o][k]
    int skip_mode;             // 0 none, 1 (fwd DQ): low-half channels x high-half K is zero, 2 (dgrad DQ): high x low
    int epilogue;
    WPtrs w;
    const float* wmin;         // lowest component pointer (hc_conv_vec_kernel addresses the others as 32-bit offsets from it)
    unsigned wspan;            // bytes from wmin to the end of the highest component tensor
    const float* src;
    const float* bias;
    float* dst;
    const float* addend;
    float* stats;
    // A second convolution of the SAME geometry in the same launch (hc_conv_vec_kernel only; nslots = 2).
    //   forward : same src, two K passes in one workgroup: the first writes {w, bias, dst, addend, stats, epilogue}, the
    //             second the *2 set (filter | gate and skip | residual of a residual block read the same tensor,
    //             model.py:121-132)
    //   dgrad   : dst = dgrad(src, w) + dgrad(src2, w2): the K loop runs over both sources in turn
    int nslots;
    int epilogue2;
    WPtrs w2;
    const float* src2;
    const float* bias2;
    float* dst2;
    const float* addend2;
    float* stats2;
};

struct WgradP {
    int algebra;
    int N, Cin, Cout;
    int inH, inW, outH, outW;
    int KH, KW;
    int sh, sw, ph, pw, dh, dw;
    int Ktot;          // Cin*KK  (columns)
    int OA, IA;
    int inS, outS;
    long long Ptot;    // N*outS  (reduction length)
    int nsplit;
    long long split_len;   // positions per split (multiple of 32: wgrad_splits; hc_wgrad_row_kernel relies on it)
    const float* x;
    const float* dy;
    WPtrsMut gw;       // component gradients (accumulated into)
    // a second weight gradient with the same x in the same launch (hc_wgrad_row_kernel only): blockIdx.y selects
    // {dy, gw} or {dy2, gw2}
    int nslots;
    const float* dy2;
    WPtrsMut gw2;
    // Fused BatchNorm+ReLU+MaxPool(ph, 1) backward (hc_wgrad_row_kernel<..., 1>): `dy` is the CONV OUTPUT y and the
    // gradient is formed while staging:  dy = y*c1[co] + dz*a[co] + c0[co],  dz = dpooled at the arg-max row of a
    // window whose pooled value is > 0, else 0.  coef = [c1 | a | c0] (3*Cout).
    const float* pooled;
    const float* dpooled;
    const unsigned char* pidx;
    const float* coef;
    int poolh;         // pooling window height
    DropP drop;        // FUSED: dpooled is the gradient behind the stage's Dropout; replay its mask (p == 0: none)
    int mz, nact, nt;  // tile enumeration without the zero quadrant: the first mz row tiles have nact column tiles, the rest nt
};

// What one forward / data-gradient call launches, decided from a filled ConvP alone (hc_conv_plan, hc_conv_fwd.hip): the
// launch, the kernel label and the pair query all read it.
struct ConvPlan {
    enum Kind { GENERAL, VEC, SMALLK } kind;   // hc_conv_kernel / hc_conv_vec_kernel / hc_conv_smallk_kernel
    int ct, pt;        // channel and position tile (SMALLK: ct only)
    int kh, kw;        // taps fixed at compile time, 0 = run-time
    int fast;          // hc_conv_kernel's FAST instantiation applies (also what VEC falls back to at launch time)
    int kc;            // VEC: K chunk (36 / 24)
    int pair;          // VEC: two convolutions in one launch (PAIRS)
};

// Weight-gradient tile configurations, indexed by wgrad_cfg() (hc_wgrad.hip): waves along rows, row tiles and column
// tiles per wave of the four waves.  The tile sizes, both template dispatches and the label text come from this table.
struct WgradTile {
    int wrw, rt, ctl;
    constexpr int bm() const { return wrw * rt * 16; }
    constexpr int bn() const { return (4 / wrw) * ctl * 16; }
};
constexpr WgradTile WGRAD_TILES[6] = {{2, 4, 4}, {4, 3, 5}, {2, 2, 2}, {2, 3, 4}, {4, 1, 5}, {4, 1, 10}};
// FN<WRW, RT, CTL>(args...) for tile configuration `cfg`
#define SELD_WGRAD_CASE(I, FN, ...) \
    case I: FN<WGRAD_TILES[I].wrw, WGRAD_TILES[I].rt, WGRAD_TILES[I].ctl>(__VA_ARGS__); break;
#define SELD_WGRAD_DISPATCH(cfg, FN, ...)                                                                             \
    switch (cfg) {                                                                                                    \
        SELD_WGRAD_CASE(0, FN, __VA_ARGS__) SELD_WGRAD_CASE(1, FN, __VA_ARGS__) SELD_WGRAD_CASE(2, FN, __VA_ARGS__)   \
        SELD_WGRAD_CASE(3, FN, __VA_ARGS__) SELD_WGRAD_CASE(4, FN, __VA_ARGS__) SELD_WGRAD_CASE(5, FN, __VA_ARGS__)   \
    }

// blockIdx.z -> (row tile, column tile), skipping the tiles that lie wholly in the dual-quaternion zero quadrant.
// The position split is blockIdx.x, the FAST dispatch index: workgroup ids go round-robin to the 8 XCDs, so with a
// split count that is a multiple of 8 all tiles of one split -- which read the same dy rows / x columns -- run on
// the same XCD and share its L2 (PMC: the 3x3 layer fetched 3.4x its operands with the tile index fastest).
__device__ __forceinline__ void wgrad_tile(const WgradP& p, int* mt, int* nt) {
    const int t = blockIdx.z, head = p.mz * p.nact;
    if (t < head) { *mt = t / p.nact; *nt = t - *mt * p.nact; }
    else { const int u = t - head; const int m = u / p.nt; *mt = p.mz + m; *nt = u - m * p.nt; }
}

// Block (p, q) of the Hamilton matrix with one index per lane and the other wave-uniform:
// returns the component, *zero for the structural zero quadrant, *neg for a negative sign.
__device__ __forceinline__ int hc_comp(int algebra, int pp, int qq, bool* zero, bool* neg) {
    *zero = false;
    *neg = false;
    if (algebra == 1) return 0;
    *neg = (0x284Eu >> (((pp & 3) << 2) | (qq & 3))) & 1u;
    int c = (pp ^ qq) & 3;
    if (algebra == 8) {
        const int hp = pp >> 2, hq = qq >> 2;
        *zero = (hp == 0 && hq == 1);
        if (hp == 1 && hq == 0) c += 4;
    }
    return c;
}

// ---- what the three block-matrix weight-gradient kernels (hc_wgrad.hip, hc_wgrad_row.hip) share: origin, column decode,
// LDS -> MFMA step, Hamilton fold.  Their staging is their own.

// Tile origin and position range of a workgroup.  CHUNK positions per staged step; WHOLE: the range is a whole number of
// steps (the row kernel: split_len and Ptot are multiples of 32), so the step count needs no round-up.
struct WgradOrigin {
    int m0, n0;                // first row (co) and column (kk) of the tile
    long long pbeg, pend;      // positions [pbeg, pend) of this split
    int nchunks;
    bool zero;                 // the tile lies wholly in the dual-quaternion zero block: rows primal (co < Cout/2), columns
                               // dual (ci >= Cin/2) -- the caller returns
};
template <int BM, int BN, int CHUNK, bool WHOLE>
__device__ __forceinline__ WgradOrigin wgrad_origin(const WgradP& p) {
    static_assert(CHUNK == 16 || CHUNK == 32, "staged step");
    WgradOrigin o;
    int tile_m, tile_n;
    wgrad_tile(p, &tile_m, &tile_n);
    o.m0 = tile_m * BM;
    o.n0 = tile_n * BN;
    o.zero = p.algebra == 8 && o.m0 + BM <= (p.Cout >> 1) && o.n0 >= (p.Ktot >> 1);
    o.pbeg = (long long)blockIdx.x * p.split_len;
    o.pend = o.pbeg + p.split_len;
    if (o.pend > p.Ptot) o.pend = p.Ptot;
    o.nchunks = o.pbeg < o.pend ? (int)((o.pend - o.pbeg + (WHOLE ? 0 : CHUNK - 1)) >> (CHUNK == 32 ? 5 : 4)) : 0;
    return o;
}

// Column kk = ci*KH*KW + kh*KW + kw of the im2col matrix; taps fixed at compile time, 0 = run-time.
template <int KH_T, int KW_T>
__device__ __forceinline__ void wgrad_col(const WgradP& p, int kk, int* ci, int* kh, int* kw) {
    const int KW = KW_T ? KW_T : p.KW;
    const int KK = (KH_T ? KH_T : p.KH) * KW;
    *ci = kk / KK;
    const int kidx = kk - *ci * KK;
    *kh = kidx / KW;
    *kw = kidx - *kh * KW;
}

// One staged step: 4 * HALVES k-groups of LDS images [k-group][row][4 positions].  Lane (fr, fk) of wave (wr, wc) reads one
// 16-byte fragment per tile and k-group, which feeds four MFMAs.  LATE_BARRIER: nothing may move across the start of the last
// k-step, so the LDS stores that follow mix with that k-step only (hc_wgrad_row_kernel).
template <int RT, int CTL, int HALVES, bool LATE_BARRIER, int AROWS, int BROWS>
__device__ __forceinline__ void wgrad_mfma_step(const float (&As)[2][4 * HALVES][AROWS][4], const float (&Bs)[2][4 * HALVES][BROWS][4],
                                                int buf, int wr, int wc, int fr, int fk, floatx4 (&acc)[RT][CTL]) {
#pragma unroll
    for (int half = 0; half < HALVES; ++half) {
        floatx4 av[RT], bv[CTL];
#pragma unroll
        for (int i = 0; i < RT; ++i) av[i] = *reinterpret_cast<const floatx4*>(&As[buf][half * 4 + fk][wr * (RT * 16) + i * 16 + fr][0]);
#pragma unroll
        for (int j = 0; j < CTL; ++j) bv[j] = *reinterpret_cast<const floatx4*>(&Bs[buf][half * 4 + fk][wc * (CTL * 16) + j * 16 + fr][0]);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (LATE_BARRIER && half == HALVES - 1 && s == 3) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < RT; ++i)
#pragma unroll
                for (int j = 0; j < CTL; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][s], bv[j][s], acc[i][j], 0, 0, 0);
        }
    }
}

// D layout: col = fr (B index = column kk), row = fk*4 + r (A index = co).  Fold the tile into the component gradients gw
// with float atomics: block (pp, qq) -> sign * dw[comp][o][c*KK + kidx].  CK = IA * KH * KW.
template <int RT, int CTL>
__device__ __forceinline__ void wgrad_fold(const WgradP& p, const WPtrsMut& gw, const floatx4 (&acc)[RT][CTL], int m0, int n0,
                                           int CK, int wr, int wc, int fr, int fk) {
    // read once: the atomics below keep the compiler from carrying a load through `p` across them
    const int algebra = p.algebra, Cout = p.Cout, Ktot = p.Ktot, OA = p.OA;
#pragma unroll
    for (int j = 0; j < CTL; ++j) {
        const int kk = n0 + wc * (CTL * 16) + j * 16 + fr;
        if (kk >= Ktot) continue;
        const int qq = kk / CK;
        const int ckl = kk - qq * CK;
#pragma unroll
        for (int i = 0; i < RT; ++i) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = m0 + wr * (RT * 16) + i * 16 + fk * 4 + r;
                if (co >= Cout) continue;
                const int pp = co / OA;
                const int o = co - pp * OA;
                bool zero, neg;
                const int comp = hc_comp(algebra, pp, qq, &zero, &neg);
                if (zero) continue;
                const float v = acc[i][j][r];
                atomicAdd(gw.p[comp] + (size_t)o * CK + ckl, neg ? -v : v);
            }
        }
    }
}

// Taps the weight-gradient kernels are specialised for: (1,1), (1,3), (3,3); anything else runs with run-time taps (0,0).
// The launches, the label and the row kernel's eligibility all read this.
inline bool wgrad_taps(const WgradP& p, int* kh, int* kw) {
    const bool fixed = (p.KH == 1 && (p.KW == 1 || p.KW == 3)) || (p.KH == 3 && p.KW == 3);
    *kh = fixed ? p.KH : 0;
    *kw = fixed ? p.KW : 0;
    return fixed;
}

inline int hc_validate(const seld_conv_desc* d) {
    if (!d) return SELD_EINVAL;
    if (d->algebra != 1 && d->algebra != 4 && d->algebra != 8) return SELD_EINVAL;
    if (d->ndim != 1 && d->ndim != 2) return SELD_EINVAL;
    if (d->groups != 1) return SELD_EUNSUPPORTED;
    if (d->N <= 0 || d->Cin <= 0 || d->Cout <= 0) return SELD_EINVAL;
    if (d->Cin % d->algebra || d->Cout % d->algebra) return SELD_EINVAL;
    for (int i = 0; i < 2; ++i)
        if (d->in[i] <= 0 || d->k[i] <= 0 || d->stride[i] <= 0 || d->dil[i] <= 0 || d->pad[i] < 0) return SELD_EINVAL;
    if (d->k[0] * d->k[1] > 255) return SELD_EUNSUPPORTED;
    // one image of either operand is addressed with 32-bit byte offsets
    if ((long long)d->Cin * d->in[0] * d->in[1] >= (1LL << 28)) return SELD_EUNSUPPORTED;
    return SELD_OK;
}

inline void hc_out_shape(const seld_conv_desc* d, int out[2]) {
    // span < 0: the dilated kernel is longer than the padded input.  C division truncates towards zero, so with
    // stride > -span the quotient would be 0 and the extent 1: report 0 (every caller treats o <= 0 as SELD_EINVAL)
    for (int i = 0; i < 2; ++i) {
        const int span = d->in[i] + 2 * d->pad[i] - d->dil[i] * (d->k[i] - 1) - 1;
        out[i] = span < 0 ? 0 : span / d->stride[i] + 1;
    }
}

// What the fast-product kernels (hcq_conv.hip, hcq_wgrad.hip) take: a 'same' convolution -- stride 1, no dilation along
// H, output extent = input extent by symmetric padding -- with 1x1, 1x3 (dilated) or 3x3 taps, both tensors below 4 GB
// (the kernels address them with 32-bit byte offsets).
inline bool hcq_same_geometry(const seld_conv_desc* d) {
    if (d->stride[0] != 1 || d->stride[1] != 1 || d->dil[0] != 1) return false;
    int o[2];
    hc_out_shape(d, o);
    if (o[0] != d->in[0] || o[1] != d->in[1]) return false;
    const int KH = d->k[0], KW = d->k[1];
    if (!((KH == 1 && (KW == 1 || KW == 3)) || (KH == 3 && KW == 3))) return false;
    if (2 * d->pad[1] != d->dil[1] * (KW - 1) || 2 * d->pad[0] != (KH - 1)) return false;
    if (KW == 1 && d->dil[1] != 1) return false;
    const long long S = (long long)d->N * d->in[0] * d->in[1] * 4;
    return S * d->Cin < 0xFFFFFFF0ll && S * d->Cout < 0xFFFFFFF0ll;
}

// ---- entry points one hc_*.hip file offers another --------------------------------------------------------------------------
// hc_wgrad_row.hip: does the row-chunk kernel take this call, and its launch for tile configuration cfg (index into WGRAD_TILES)
bool hc_wgrad_row_ok(const WgradP& p);
void hc_wgrad_row_launch(const WgradP& p, int cfg, hipStream_t st);
// hc_wgrad.hip: the kernel a weight gradient launches, whether a pair launch would run, and the weight gradient reduced over
// the output extent o
int hc_wgrad_label(const seld_conv_desc* d, char* buf, int buflen);
int hc_wgrad_pair_ok(const seld_conv_desc* d);
int hc_wgrad_out(const seld_conv_desc* d, const int o[2], const float* x, const float* dy, float* const dw[8], void* det_ws,
                 size_t det_bytes, hipStream_t st);
// hc_conv_fwd.hip: the forward convolution evaluated on the output extent o
int hc_conv_fwd_out(const seld_conv_desc* d, const int o[2], const float* x, const float* const w[8], float* y, hipStream_t st);

}  // namespace seld
