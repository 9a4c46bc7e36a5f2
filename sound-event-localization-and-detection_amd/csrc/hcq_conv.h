// What the fast-product convolution files share: the launch arguments and the plan (hcq_conv.hip plans, hcq_conv.hip and
// hcq_first.hip launch), the instantiation table with its dispatch macros, and the device pieces that more than one kernel
// is made of -- block order, channel decode and statistics flush for the convolution kernels; tile origin, staging and
// tap decode for the two row-walking first-layer kernels of hcq_first.hip.
#pragma once
#include <string.h>
#include <type_traits>
#include "hc_common.h"
#include "hcq_forms.h"

namespace seld {

// The channel-tile layout of a launch, shared by the convolution kernels and the kernel that packs their weights.
struct HcqTiles {
    int NT1, NT2, NR;            // tiles active in range 0 only / in both ranges; K ranges (1 quaternion, 2 dual quaternion)
    int nreg, mix;               // regular channel tiles per weight set; 1: a mixed 8 + 8 tile follows them
    int ob_step;                 // block channels a channel tile advances by (16 / 32, or 0 for the single-tile layout)
    int half_src[2];             // source half (0 primal, 1 dual) read by range 0 / range 1
    int tile_half[3][2];         // tile t, 8-channel group g: destination half ...
    int tile_ob[3][2];           // ... and first block channel (-1: padding, nothing stored); tile 2 = the mixed tile
    long long range_stride[2];   // floats of one (chunk, range) block of the packed weights
    long long ytile_stride;      // floats of one regular channel tile (all chunks of all sources)
    long long set_stride;        // floats of one weight set (regular tiles + the mixed tile's block)
};

struct HcqP {
    const float* src;
    const float* src2;           // data gradient of a pair: dst = dgrad(src, W_0) + dgrad(src2, W_1), the K loop runs over both
    int nsrc;                    // 1 or 2
    int mix_ytile;               // index of the channel tile that holds ONLY the mixed 8 + 8 tile (dual quaternion with
                                 // 24 block channels), or -1
    const float* wpack;
    float* dst[2];               // per weight set (a pair launch computes two convolutions of the same input)
    const float* bias[2];
    const float* addend[2];
    float* stats[2];
    int epilogue[2];
    int A;                       // 4 or 8
    int N, Csrc, Cdst;           // channels of src / of ONE dst
    int IB, OB;                  // Csrc / A, Cdst / A
    int W;                       // row length (T of a 1-D layer, image width of a 2-D layer)
    int Himg;                    // image height (1 for 1-D)
    int dil, dpad;               // dilation along W, padded up to a multiple of 4 (the halo each side of a tile)
    int wext;                    // 64 + 2 * dpad
    int nch;                     // K chunks per range (IB / IBC)
    int ytiles;                  // channel tiles per weight set (t.nreg + t.mix)
    HcqTiles t;
    int ring_off;                // hcq_conv_kernel: byte offset of the fragment ring in LDS (behind the input buffers)
    int half_slots;              // ring slot = 8 forms of a pair of k-groups (0) or 4 forms (1: half the ring, one more barrier)
};

// hcq_first_pool_kernel (hcq_first.hip)
struct HcqPoolP {
    const float* gamma;          // (Cdst)
    float* pool_raw;             // (N, Cdst, Himg / 8, W): the conv output at the window's arg-max / arg-min row
    unsigned char* idx;          // same shape: that row (0..7)
    // FIN: BatchNorm with KNOWN statistics (first_stage.hip: from the input's second moments), ReLU and the stage's Dropout
    // applied to the window value before it is stored: out = relu(a raw + b) * mask; pool_raw is then written only for
    // channels with gamma == 0 (the one case in which the backward pass cannot recover xhat from out)
    const float* beta;
    const float* mean;
    const float* invstd;
    float* out;
    DropP drop;
};

// hcq_pack_kernel / hcq_pack_flat_kernel (hcq_conv.hip)
struct HcqPackP {
    WPtrs w[2];                  // component tensors (OA, IA, taps) of the 1 or 2 weight sets
    float* out;
    int A, mode;
    int OA, IA, taps;            // of the CONVOLUTION (not swapped for the data gradient)
    int IBC, nch, NG, NPAIR;
    int nsets;                   // forward pairs: separate outputs
    int nsrc;                    // gradient pairs: two (source, weight set) along K
    HcqTiles t;
    long long total;
};

typedef unsigned int uintx4h __attribute__((ext_vector_type(4)));

// n / d for 0 <= n < 2^20 with a precomputed 1.0f / d (exact: see hc_conv_vec.hip)
__device__ __forceinline__ int small_div_h(int n, float inv_d) { return (int)(((float)n + 0.5f) * inv_d); }

// ---------------------------------------------------------------------------------------------------------------------
// device pieces of all three convolution kernels
// ---------------------------------------------------------------------------------------------------------------------
// Workgroups go round-robin to the 8 XCDs, each with its own L2: give every XCD a contiguous range of position tiles.
// The tiles that share halo rows and output lines then meet in one L2, and the 64-column pieces of one 2 KB image row
// are written back by ONE L2 (spread over eight, every piece was a separate 256-byte DRAM write).
__device__ __forceinline__ unsigned hcq_xcd_block() {
    return (gridDim.x & 7u) ? blockIdx.x : (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
}

// First-component channel of the lane with fragment row fr (8-channel group grp = fr >> 3) in the tile of descriptor
// slot `slot`; component q is OB channels further each.  -1: padding (slot < 0, or the group holds no channels).
__device__ __forceinline__ int hcq_lane_channel(const HcqTiles& t, int slot, int grp, int fr, int OB) {
    if (slot < 0) return -1;
    const int ob0 = t.tile_ob[slot][grp];
    return ob0 >= 0 ? t.tile_half[slot][grp] * 4 * OB + ob0 + (fr & 7) : -1;
}

// BatchNorm statistics of a workgroup from its LDS scratch to the launch's replica rows: one thread per (tile,
// component, channel of 16), two atomics.  The kernel's own slot layout comes as slot_of(wave, k, t, q, fr): the float
// index in `buf` of the k-th partial sum (of NK) that wave `wave` left for that channel, its sum of squares s2_off floats
// behind.  They are added wave by wave (0..3), k by k: the order of the additions is part of the result's bits.
// mix_slot >= 0 (hcq_conv_kernel's mixed-tile workgroups): that accumulator slot is descriptor slot 2, the others are
// padding.  ch_add: first channel of the workgroup's channel tile.
template <int NT, int NK, typename SlotOf>
__device__ __forceinline__ void hcq_stats_flush(const HcqP& p, int set, int tid, int mix_slot, int ch_add, const float* buf,
                                                int s2_off, SlotOf slot_of) {
    __syncthreads();
    float* rep = p.stats[set] + (size_t)(blockIdx.x % SELD_STATS_REPLICAS) * 2 * p.Cdst;
    for (int e = tid; e < NT * 4 * 16; e += 256) {
        const int fr = e & 15, q = (e >> 4) & 3, t = e >> 6;
        const int chb = hcq_lane_channel(p.t, mix_slot < 0 ? t : (t == mix_slot ? 2 : -1), fr >> 3, fr, p.OB);
        if (chb < 0) continue;
        const int chn = chb + q * p.OB + ch_add;
        float a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv)
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int s = slot_of(wv, k, t, q, fr);
                a1 += buf[s];
                a2 += buf[s + s2_off];
            }
        atomicAdd(rep + chn, a1);
        atomicAdd(rep + p.Cdst + chn, a2);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// device pieces of the row-walking first-layer kernels (hcq_first.hip): 3x3 taps, dilation 1, a workgroup keeps its 64
// columns and walks R image rows over XR = R + 2 staged input rows of 72 floats (halo of 4 each side; the host checks
// p.wext)
// ---------------------------------------------------------------------------------------------------------------------
constexpr int HCQ_FIRST_WEXT = 72, HCQ_FIRST_DPAD = 4;

struct HcqFirstOrigin { int w0, hq, h0, n_img; };      // first column, row block and its first row, image

template <int R>
__device__ __forceinline__ HcqFirstOrigin hcq_first_origin(const HcqP& p) {
    const unsigned tiles_per_row = (unsigned)p.W >> 6;
    const unsigned hblocks = (unsigned)p.Himg / R;
    unsigned b = hcq_xcd_block();
    HcqFirstOrigin o;
    o.w0 = (int)(b % tiles_per_row) * 64;
    b /= tiles_per_row;
    o.hq = (int)(b % hblocks);
    o.h0 = o.hq * R;
    o.n_img = (int)(b / hblocks);
    return o;
}

// Stage the XR rows of every (component, block channel) once: LDS image [component][block channel][row][72].
template <int IBC, int XR>
__device__ __forceinline__ void hcq_first_stage_rows(float* lds, const HcqP& p, const HcqFirstOrigin& o, int tid) {
    constexpr int qw = HCQ_FIRST_WEXT >> 2;
    const unsigned S = (unsigned)(p.Himg * p.W);
    const unsigned src_bytes = (unsigned)p.N * (unsigned)p.Csrc * S * 4u;
    const unsigned OOB = 0xFFFFFFF0u;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)p.src, 0, src_bytes, 0x00020000);
    const int items = p.A * IBC * XR * qw;
    const unsigned img_base = (unsigned)o.n_img * (unsigned)p.Csrc * S;
    constexpr float inv_qw = 1.0f / (float)qw;
    // four requests in flight per thread, then their four LDS stores (one load -> wait -> store per iteration exposed a
    // first-touch memory latency six to twelve times at the head of every workgroup)
    for (int f0 = tid; f0 < items; f0 += 4 * 256) {
        uintx4h v[4];
        int dst_[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int f = f0 + 256 * u;
            const int row = small_div_h(f, inv_qw);               // (comp * IBC + ibl) * XR + xr
            const int quad = f - row * qw;
            const int ci = row / XR;
            const int xr = row - ci * XR;
            const int comp = ci / IBC;
            const int ibl = ci - comp * IBC;
            const int hh = o.h0 - 1 + xr;
            const int ww = o.w0 - HCQ_FIRST_DPAD + 4 * quad;
            const bool ok = f < items && (unsigned)hh < (unsigned)p.Himg && (unsigned)ww < (unsigned)p.W;
            const unsigned e = img_base + ((unsigned)(comp * p.IB + ibl) * (unsigned)p.Himg + (unsigned)hh) * (unsigned)p.W + (unsigned)ww;
            v[u] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, ok ? e * 4u : OOB, 0, 0);
            dst_[u] = f < items ? (row * qw + quad) * 4 : -1;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (dst_[u] >= 0)
                *reinterpret_cast<float4*>(lds + dst_[u]) =
                    make_float4(__uint_as_float(v[u][0]), __uint_as_float(v[u][1]), __uint_as_float(v[u][2]), __uint_as_float(v[u][3]));
    }
}

// k-groups of the one K chunk (the last one padded: packed weights are zero there, the lane re-reads k = 0) ...
constexpr int hcq_first_ng(int IBC) { return (IBC * 9 + 3) / 4; }

// ... and the A-operand address of this lane in k-group g: k = 4 g + fk -> (block channel, kh, kw), as an offset into the
// staged rows of component 0 at the workgroup's row 0; a component is IBC * XR * 72 floats further, a row 72.
// (One value per call: filled through a reference to the kernel's array, two instantiations allocate other registers.)
template <int IBC, int XR>
__device__ __forceinline__ int hcq_first_tap(int g, int wave, int fr, int fk) {
    const int kq = (4 * g + fk) < IBC * 9 ? 4 * g + fk : 0;
    const int ibl = kq / 9;
    const int tap = kq - ibl * 9;
    const int kh = tap / 3;
    const int kw = tap - kh * 3;
    return (ibl * XR + kh) * HCQ_FIRST_WEXT + HCQ_FIRST_DPAD + wave * 16 + fr + (kw - 1);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
// The instantiations, once: taps, K chunk, staging items per thread of the dual-quaternion and of the quaternion kernels
// (0: none).  XI is fixed by (taps, IBC, algebra) except for the dilated 1x3 layers (halo width): a plan takes the first
// row whose XI is enough.
struct HcqInst { int KH, KW, IBC, XI8, XI4; };
constexpr HcqInst HCQ_INST[] = {{1, 3, 8, 5, 3},  {1, 3, 8, 7, 5},   {1, 3, 8, 9, 0}, {1, 3, 4, 6, 3}, {1, 1, 16, 8, 4},
                                  {1, 1, 24, 12, 6}, {1, 1, 8, 4, 2},   {3, 3, 4, 7, 4}, {3, 3, 2, 4, 2}, {3, 3, 1, 2, 1}};
// ... and the channel-tile programs every row exists in (MX: launches with mixed-tile workgroups)
struct HcqTileV { int NT1, NT2, NR; bool MX; };
constexpr HcqTileV HCQ_TILEV[] = {{1, 2, 2, false}, {1, 1, 2, true}, {1, 1, 2, false}, {2, 0, 1, false}, {1, 0, 1, false}};
constexpr int HCQ_FIRST_R = 8;   // image rows per workgroup of hcq_first_kernel / hcq_first_pool_kernel (a pooling window)

constexpr int HCQ_NINST = sizeof(HCQ_INST) / sizeof(HCQ_INST[0]), HCQ_NTILEV = sizeof(HCQ_TILEV) / sizeof(HCQ_TILEV[0]);

// FN<row, variant>::run(args...) for the (row, variant) a plan resolved
static_assert(HCQ_NINST == 10 && HCQ_NTILEV == 5, "SELD_HCQ_DISPATCH lists the rows 0..9 and the tile programs 0..4");
#define SELD_HCQ_V(I, FN, ...)                                                          \
    case I:                                                                             \
        switch (pl.variant) {                                                           \
            case 0: return FN<I, 0>::run(__VA_ARGS__);                                  \
            case 1: return FN<I, 1>::run(__VA_ARGS__);                                  \
            case 2: return FN<I, 2>::run(__VA_ARGS__);                                  \
            case 3: return FN<I, 3>::run(__VA_ARGS__);                                  \
            case 4: return FN<I, 4>::run(__VA_ARGS__);                                  \
        }                                                                               \
        break;
#define SELD_HCQ_DISPATCH(FN, ...)                                                                                     \
    switch (pl.row) {                                                                                                  \
        SELD_HCQ_V(0, FN, __VA_ARGS__) SELD_HCQ_V(1, FN, __VA_ARGS__) SELD_HCQ_V(2, FN, __VA_ARGS__)                   \
        SELD_HCQ_V(3, FN, __VA_ARGS__) SELD_HCQ_V(4, FN, __VA_ARGS__) SELD_HCQ_V(5, FN, __VA_ARGS__)                   \
        SELD_HCQ_V(6, FN, __VA_ARGS__) SELD_HCQ_V(7, FN, __VA_ARGS__) SELD_HCQ_V(8, FN, __VA_ARGS__)                   \
        SELD_HCQ_V(9, FN, __VA_ARGS__)                                                                                 \
    }

// Everything the entry points need to know about (desc, mode, npair): which kernel, its grid and LDS, its arguments and
// the arguments of the kernel that packs its weights.
struct HcqPlan {
    int ok;
    int row, variant;            // HCQ_INST / HCQ_TILEV
    int XI;                      // of the instantiation
    bool gf;                     // hcq_conv_kernel with per-wave global fragment loads (no ring)
    int first_rows;              // > 0: hcq_first_kernel (pool: hcq_first_pool_kernel) walks this many image rows per workgroup
    bool pool;
    HcqP kp;
    HcqPackP pp;
    size_t pack_floats;
    dim3 grid;
    size_t smem;
};

// hcq_conv.hip.  mode 0 forward (npair: 1 or 2 convolutions of the same input -> separate outputs),
// mode 1 data gradient (npair: 1, or 2 = sum of the gradients of two convolutions w.r.t. their common input).
// mode 2 = mode 0 for the pooling first-stage kernel (hcq_first_pool_kernel): same packed forms, and the 8-channel
// dual-quaternion layer is NOT left to the short-K kernel.
// first_ok = false: never the row-walking first-layer kernel (it takes no addend / accumulate epilogue).
HcqPlan hcq_plan(const seld_conv_desc* d, int mode, int npair, bool first_ok = true);
// hcq_first.hip: the launch of a plan with first_rows > 0 and no pooling
int hcq_launch_first(const HcqPlan& pl, hipStream_t st);

template <typename Kern, typename... Args>
static int hcq_launch_kernel(Kern kern, const HcqPlan& pl, hipStream_t st, const Args&... args) {
    if (pl.smem > 64 * 1024 &&
        hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.smem) != hipSuccess)
        return SELD_ELAUNCH;
    hipLaunchKernelGGL(kern, pl.grid, dim3(256), pl.smem, st, args...);
    return check_launch();
}

}  // namespace seld
