// The first layers of the fast-product convolution (3x3, one or two input block channels; gfx950): hcq_first_kernel and
// hcq_first_pool_kernel, their launchers and the seld_hcq_first_pool* entry points.  Forms, packed weights and plan are
// those of hcq_conv.hip.
//
// The K loop of a first layer is ONE short chunk (9 or 18 k of 12 / 20 slots), so hcq_conv_kernel is all prologue and
// epilogue there (120 MFMAs per workgroup: 688 us for the 8-channel layer at batch 32, the block-matrix short-K kernel
// takes 609).  Here a workgroup keeps its 64 columns and walks R consecutive image rows: the R + 2 input rows are staged
// once (23 / 46 KB), there is ONE barrier, the weight fragments of row r+1 are requested under the MFMAs of row r, a
// row's stores drain under the next row's MFMAs and the BatchNorm statistics stay on chip until the last row.
//
// Both kernels are the same row walk.  Written once, in hcq_conv.h: block order and tile origin (hcq_first_origin),
// staging (hcq_first_stage_rows), tap decode (hcq_first_tap), channel decode (hcq_lane_channel) and -- for
// hcq_first_kernel -- the statistics flush (hcq_stats_flush).  A kernel keeps what is its own:
//                        hcq_first_kernel                              hcq_first_pool_kernel
//   weight fragments     bfr[8][NT], per-lane global loads             bfr[8] of ONE tile, from an LDS copy filled per tile
//   a wave runs          all NT channel tiles per row                  one tile for all R rows, then the next
//   accumulators         [NT][8]                                       [8]
//   epilogue of a row    store y; statistics in lane-private LDS slots store y (WY) + statistics in registers; window maximum
//   at the end           --                                            window value + row; FIN: BatchNorm, ReLU, Dropout
//   workgroups per CU    2                                             3
// and, because the register allocation of these kernels (up to 254 of 256, 168 of 168) does not survive it, its own copy
// of the loop over a row's k-groups, and the pooling kernel its own statistics flush ("Fast-product first
// layers").
#include "hcq_conv.h"

namespace seld {

template <int IBC, int NT1, int NT2, int NR, int R>
__global__ __launch_bounds__(256, 2) void hcq_first_kernel(const HcqP p) {
    constexpr int NT = NT1 + NT2;
    constexpr int NG = hcq_first_ng(IBC);
    constexpr int NPAIR = (NG + 1) / 2;
    constexpr int NPC = NR * NPAIR;
    constexpr int XR = R + 2;                         // staged input rows
    constexpr int wext = HCQ_FIRST_WEXT;
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fk = lane >> 4;
    const int A = p.A;

    const HcqFirstOrigin o = hcq_first_origin<R>(p);
    const int w0 = o.w0, h0 = o.h0, n_img = o.n_img;
    const unsigned S = (unsigned)(p.Himg * p.W);
    hcq_first_stage_rows<IBC, XR>(lds, p, o, tid);

    int aoff[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) aoff[g] = hcq_first_tap<IBC, XR>(g, wave, fr, fk);
    constexpr int comp_stride = IBC * XR * wext;
    const float* const wbase = p.wpack;                 // one channel tile, one weight set, one chunk

    float2 bfr[8][NT];
    float gm[2][8];
    float raw[4];
    auto load_b1 = [&](const float* blk, int j, int m, auto ntrc) __attribute__((always_inline)) {
        constexpr int NTR = decltype(ntrc)::value;
        const float* q = blk + ((long long)(j * 8 + m) * 64 + lane) * (2 * NTR);
#pragma unroll
        for (int t = 0; t < NTR; ++t) bfr[m][t] = *reinterpret_cast<const float2*>(q + 2 * t);
    };
    auto read_raw = [&](const float* xs, int g) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) raw[q] = xs[aoff[g] + q * comp_stride];
    };
    using INT = std::integral_constant<int, NT>;
    using INT2 = std::integral_constant<int, NT2>;

    float* const dst = p.dst[0];
    const float* const bias = p.bias[0];
    const int epi = p.epilogue[0];
    const int grp = fr >> 3;
    const unsigned img_off = (unsigned)n_img * (unsigned)p.Cdst * S;
    // BatchNorm statistics: one slot per (wave, tile, component, LANE) behind the staged rows, read-modify-written row by
    // row by its owner (24 more registers per lane would spill; LDS float atomics doubled the kernel's time)
    float* const sbuf = lds + A * IBC * XR * wext;
    const bool want_stats = (epi & SELD_EPI_STATS) != 0;
    if (want_stats)
        for (int e = tid; e < 4 * NT * 4 * 64 * 2; e += 256) sbuf[e] = 0.f;
    int chbase[NT];                                     // first-component channel of this lane in tile t, -1: padding
#pragma unroll
    for (int t = 0; t < NT; ++t) chbase[t] = hcq_lane_channel(p.t, t, grp, fr, p.OB);

#pragma unroll
    for (int m = 0; m < 8; ++m) load_b1(wbase, 0, m, INT{});
    __syncthreads();

#pragma unroll 1
    for (int r = 0; r < R; ++r) {
        floatx4 acc[NT][8];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int m = 0; m < 8; ++m) acc[t][m] = (floatx4){0.f, 0.f, 0.f, 0.f};
        const bool more = r + 1 < R;
        // the fragments are the same for every row: without this the compiler hoists all 160 registers of them out of
        // the row loop (414 VGPRs wanted)
        const float* wrow = wbase;
        asm volatile("" : "+s"(wrow));
        const float* xs0 = lds + r * wext + p.t.half_src[0] * 4 * comp_stride;
        const float* xs1 = lds + r * wext + p.t.half_src[1] * 4 * comp_stride;
        read_raw(xs0, 0);
        hcq_xforms(raw, gm[0]);
        // The row's k-groups: hcq_conv_kernel's global-load loop (pipeline and scheduling barriers: see there).  The same
        // loop stands in hcq_first_pool_kernel, for one tile: a change here is made there too.  (As one shared function
        // five instantiations of this kernel allocate 2 to 8 registers fewer -- DESIGN.md.)
#pragma unroll
        for (int s = 0; s < NR * NG; ++s) {
            const int rr = s / NG, g = s - rr * NG;
            const int pc = rr * NPAIR + g / 2;
            const int gst = s & 1;
            const bool last = s + 1 == NR * NG;
            const bool pair_ends = (g & 1) == 1 || g + 1 == NG;
            if (!last) {
                const int rn = (s + 1) / NG, gn = (s + 1) - rn * NG;
                read_raw(rn == 0 ? xs0 : xs1, gn);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                if (rr == 0) {
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        acc[t][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(gm[gst][m], (g & 1) ? bfr[m][t].y : bfr[m][t].x,
                                                                          acc[t][m], 0, 0, 0);
                } else {
#pragma unroll
                    for (int t = 0; t < NT2; ++t)
                        acc[NT1 + t][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(gm[gst][m], (g & 1) ? bfr[m][t].y : bfr[m][t].x,
                                                                                acc[NT1 + t][m], 0, 0, 0);
                }
                if (pair_ends) {
                    const int pn = pc + 1;
                    if (pn < NPC) {
                        const int rn = pn / NPAIR, jn = pn - rn * NPAIR;
                        if (rn == 0) load_b1(wrow, jn, m, INT{});
                        else load_b1(wrow + p.t.range_stride[0], jn, m, INT2{});
                    } else if (more) {
                        load_b1(wrow, 0, m, INT{});               // the next row starts with the same fragments
                    }
                }
            }
            if (!last) hcq_xforms(raw, gm[gst ^ 1]);
            __builtin_amdgcn_sched_barrier(0);
        }
        // ---- this row's results ------------------------------------------------------------------------------------
        const unsigned pos_off = (unsigned)(h0 + r) * (unsigned)p.W + (unsigned)(w0 + wave * 16 + fk * 4);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            floatx4 c[4];
            hcq_recombine4(acc[t], c);
            if (chbase[t] >= 0) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int chn = chbase[t] + q * p.OB;
                    const float bq = bias ? bias[chn] : 0.f;
                    const float4 o4 = make_float4(c[q][0] + bq, c[q][1] + bq, c[q][2] + bq, c[q][3] + bq);
                    *reinterpret_cast<float4*>(dst + img_off + (unsigned)chn * S + pos_off) = o4;
                    if (want_stats) {
                        const int slot = ((wave * NT + t) * 4 + q) * 64 + lane;
                        sbuf[slot] += (o4.x + o4.y) + (o4.z + o4.w);                   // the slot is this lane's own
                        sbuf[4 * NT * 4 * 64 + slot] += (o4.x * o4.x + o4.y * o4.y) + (o4.z * o4.z + o4.w * o4.w);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);           // one tile's recombination at a time (registers)
        }
    }

    if (want_stats)      // per channel: the waves in order, in each its four lanes (fk) in order
        hcq_stats_flush<NT, 4>(p, 0, tid, -1, 0, sbuf, 4 * NT * 4 * 64,
                               [](int wv, int k4, int t, int q, int fr_) __attribute__((always_inline)) {
                                   return ((wv * NT + t) * 4 + q) * 64 + k4 * 16 + fr_;
                               });
}

// ---------------------------------------------------------------------------------------------------------------------
// First stage with the pooling decision fused in: conv -> [BatchNorm2d -> ReLU ->] MaxPool2d(8, 1).  BatchNorm + ReLU is
// z = relu(a y + b) with a = gamma * invstd, and invstd > 0: the SIGN of a is the sign of gamma, known before the batch
// statistics are.  So the maximum of z over a pooling window sits where y is largest (gamma > 0) or smallest (gamma < 0),
// and the convolution kernel -- whose workgroup walks exactly the 8 rows of a window -- can pick that element itself:
// it writes y (the backward pass needs it), the BatchNorm statistics, and per window the chosen raw value + its row.
// A pooled-size kernel (seld_bn_pool_finish) then applies relu(a v + b) once the statistics are final; the 1.6 GB
// read-back of y by bn_relu_pool_fwd disappears.  (Ties: where the window's maximum of z is 0 every position ties and
// torch takes the first; the element chosen here may differ, but ReLU's derivative is 0 there, so no gradient does.
// gamma == 0 keeps row 0, as torch's first-maximum rule does.)
//
// Unlike hcq_first_kernel a wave finishes one channel tile for all 8 rows before the next (the running window maximum of
// three tiles at once does not fit the register file): 8 accumulators instead of 24, the sums G_m recomputed per tile.
//
// WY = false: y is not written and no statistics are gathered (csrc/first_stage.hip: the statistics come from the input's
// second moments, the backward pass never reads y) -- the kernel's only output is the pooled-size window value + row.
// ---------------------------------------------------------------------------------------------------------------------
template <int IBC, int NT1, int NT2, int NR, int R, bool WY, bool FIN = false>
__global__ __launch_bounds__(256, 3) void hcq_first_pool_kernel(const HcqP p, const HcqPoolP pp) {
    static_assert(!(WY && FIN), "the finishing variant knows the statistics beforehand: it never writes y");
    constexpr int NT = NT1 + NT2;
    constexpr int NG = hcq_first_ng(IBC);
    constexpr int NPAIR = (NG + 1) / 2;
    constexpr int XR = R + 2;
    constexpr int wext = HCQ_FIRST_WEXT;
    static_assert(R == 8, "one workgroup = one MaxPool2d(8, 1) window");
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fk = lane >> 4;
    const int A = p.A;

    const HcqFirstOrigin o = hcq_first_origin<R>(p);
    const int w0 = o.w0, hq = o.hq, h0 = o.h0, n_img = o.n_img;
    const unsigned hblocks = (unsigned)p.Himg / R;
    const unsigned S = (unsigned)(p.Himg * p.W);
    hcq_first_stage_rows<IBC, XR>(lds, p, o, tid);

    int aoff[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) aoff[g] = hcq_first_tap<IBC, XR>(g, wave, fr, fk);
    constexpr int comp_stride = IBC * XR * wext;
    float* const sred = lds + A * IBC * XR * wext;      // statistics: [tile][wave][component][16 channels][2]
    // The current tile's weight fragments live in LDS ([pair][form][lane] float2): with them in global memory every row
    // ended on `s_waitcnt vmcnt` for its fragment loads -- and loads and stores retire in order on one counter, so each
    // row also waited for the previous row's 12 stores to reach memory: store time ADDED to compute time (686 us).  With no
    // global load inside the row loop the stores drain under the next rows' MFMAs.
    float2* const wl = reinterpret_cast<float2*>(sred + NT * 4 * 4 * 16 * 2);
    const float* const wbase = p.wpack;
    float* const dst = p.dst[0];
    const float* const bias = p.bias[0];
    const bool want_stats = WY && (p.epilogue[0] & SELD_EPI_STATS) != 0;
    const int grp = fr >> 3;
    const unsigned img_off = (unsigned)n_img * (unsigned)p.Cdst * S;
    const unsigned PS = (unsigned)hblocks * (unsigned)p.W;                   // pooled plane
    const unsigned pool_off = (unsigned)n_img * (unsigned)p.Cdst * PS + (unsigned)hq * (unsigned)p.W +
                              (unsigned)(w0 + wave * 16 + fk * 4);
    __syncthreads();

    float2 bfr[8];
    float gm[2][8];
    float raw[4];
    auto read_raw = [&](const float* xs, int g) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 4; ++q) raw[q] = xs[aoff[g] + q * comp_stride];
    };

    auto tile_body = [&](auto tc) __attribute__((always_inline)) {
        constexpr int T = decltype(tc)::value;
        constexpr bool BOTH = NR == 2 && T >= NT1;            // this tile's channels take the second K range too
        constexpr int NRT = BOTH ? 2 : 1;
        constexpr int NPCT = NRT * NPAIR;
        const int chb = hcq_lane_channel(p.t, T, grp, fr, p.OB);
        // fragments of tile T only (range 0 blocks hold NT tiles per (pair, form, lane), range 1 blocks NT2): into LDS
        __syncthreads();                                  // everybody is done with the previous tile's fragments
        {
            // all of a thread's loads first, then its stores: as one load -> wait -> store per iteration the fill exposed
            // 4 / 8 / 8 cache latencies per tile, a fifth of the workgroup's time
            constexpr int NIT = NPCT * 8 * 64 / 256;
            float2 tmp[NIT];
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int e = tid + 256 * it;
                const int ln = e & 63, jm = e >> 6;       // jm = pair * 8 + form over both ranges
                const int rr = jm / (NPAIR * 8), jm0 = jm - rr * (NPAIR * 8);
                const float* blk = rr == 0 ? wbase : wbase + p.t.range_stride[0];
                const int ntr = rr == 0 ? NT : NT2, tt = rr == 0 ? T : T - NT1;
                tmp[it] = *reinterpret_cast<const float2*>(blk + ((long long)jm0 * 64 + ln) * (2 * ntr) + 2 * tt);
            }
#pragma unroll
            for (int it = 0; it < NIT; ++it) wl[tid + 256 * it] = tmp[it];
        }
        __syncthreads();
        auto load_b1 = [&](int pc, int m) __attribute__((always_inline)) { bfr[m] = wl[(pc * 8 + m) * 64 + lane]; };
        float sg[4], yb[4][4], sb[4][4], s1[4], s2[4], bq[4];     // sb = sg * yb, the key the window maximum is taken over
        unsigned bi[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float gq = chb >= 0 ? pp.gamma[chb + q * p.OB] : 1.f;
            bq[q] = (bias && chb >= 0) ? bias[chb + q * p.OB] : 0.f;
            sg[q] = gq > 0.f ? 1.f : (gq < 0.f ? -1.f : 0.f);
            s1[q] = 0.f; s2[q] = 0.f; bi[q] = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) { yb[q][e] = 0.f; sb[q][e] = -INFINITY; }
        }
#pragma unroll
        for (int m = 0; m < 8; ++m) load_b1(0, m);
#pragma unroll 1
        for (int r = 0; r < R; ++r) {
            floatx4 acc[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) acc[m] = (floatx4){0.f, 0.f, 0.f, 0.f};
            const bool more = r + 1 < R;
            const float* xs0 = lds + r * wext + p.t.half_src[0] * 4 * comp_stride;
            const float* xs1 = lds + r * wext + p.t.half_src[1] * 4 * comp_stride;
            read_raw(xs0, 0);
            hcq_xforms(raw, gm[0]);
            // hcq_first_kernel's loop over the row's k-groups, for ONE tile in the NRT ranges it takes and with the
            // fragments from their LDS copy
#pragma unroll
            for (int s = 0; s < NRT * NG; ++s) {
                const int rr = s / NG, g = s - rr * NG;
                const int pc = rr * NPAIR + g / 2;
                const int gst = s & 1;
                const bool last = s + 1 == NRT * NG;
                const bool pair_ends = (g & 1) == 1 || g + 1 == NG;
                if (!last) {
                    const int rn = (s + 1) / NG, gn = (s + 1) - rn * NG;
                    read_raw(rn == 0 ? xs0 : xs1, gn);
                }
                __builtin_amdgcn_sched_barrier(0);      // (without the two barriers of a group: 710 us against 670-690)
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(gm[gst][m], (g & 1) ? bfr[m].y : bfr[m].x, acc[m], 0, 0, 0);
                    if (pair_ends) {
                        const int pn = pc + 1;
                        if (pn < NPCT) load_b1(pn, m);
                        else if (more) load_b1(0, m);
                    }
                }
                if (!last) hcq_xforms(raw, gm[gst ^ 1]);
                __builtin_amdgcn_sched_barrier(0);
            }
            // ---- this row of this tile: components, store, statistics, window maximum ------------------------------
            floatx4 c[4];
            hcq_recombine4(acc, c);
            if (chb >= 0) {
                const unsigned pos_off = (unsigned)(h0 + r) * (unsigned)p.W + (unsigned)(w0 + wave * 16 + fk * 4);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int chn = chb + q * p.OB;
                    float o4[4] = {c[q][0], c[q][1], c[q][2], c[q][3]};
                    if (bias) { o4[0] += bq[q]; o4[1] += bq[q]; o4[2] += bq[q]; o4[3] += bq[q]; }
                    if constexpr (WY) {
                        *reinterpret_cast<float4*>(dst + img_off + (unsigned)chn * S + pos_off) = make_float4(o4[0], o4[1], o4[2], o4[3]);
                        s1[q] += (o4[0] + o4[1]) + (o4[2] + o4[3]);
                        s2[q] += (o4[0] * o4[0] + o4[1] * o4[1]) + (o4[2] * o4[2] + o4[3] * o4[3]);
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        // first maximum wins, NaN propagates: "not (key <= best)" is true for a larger key and for NaN, and
                        // for row 0 (best = -inf); gamma == 0 makes every key 0, so row 0 stays
                        const float so = sg[q] * o4[e];
                        const bool take = !(so <= sb[q][e]);
                        yb[q][e] = take ? o4[e] : yb[q][e];
                        sb[q][e] = take ? so : sb[q][e];
                        bi[q] = take ? ((bi[q] & ~(0xFFu << (8 * e))) | ((unsigned)r << (8 * e))) : bi[q];
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (chb >= 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned po = pool_off + (unsigned)(chb + q * p.OB) * PS;
                *reinterpret_cast<unsigned*>(pp.idx + po) = bi[q];
                if constexpr (FIN) {
                    const int chn = chb + q * p.OB;
                    const float gq = pp.gamma[chn];
                    const float a = gq * pp.invstd[chn], bb = pp.beta[chn] - pp.mean[chn] * a;
                    float z[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float v = yb[q][e];
                        z[e] = fmaxf(v * a + bb, 0.f);
                        if (v != v) z[e] = v;                                   // NaN propagates (torch's relu / max_pool)
                    }
                    if (pp.drop.p > 0.f) {       // the mask seld_dropout_fwd draws for element group po / 4 of `out`
                        const uint64_t off = pp.drop.offset + (pp.drop.state ? pp.drop.state[0] : 0ull);
                        const float4 mk = dropout_mask4(off + (uint64_t)(po >> 2), pp.drop.seed, pp.drop.p, pp.drop.scale);
                        z[0] = mk.x != 0.f ? z[0] * mk.x : 0.f;
                        z[1] = mk.y != 0.f ? z[1] * mk.y : 0.f;
                        z[2] = mk.z != 0.f ? z[2] * mk.z : 0.f;
                        z[3] = mk.w != 0.f ? z[3] * mk.w : 0.f;
                    }
                    *reinterpret_cast<float4*>(pp.out + po) = make_float4(z[0], z[1], z[2], z[3]);
                    if (gq == 0.f) *reinterpret_cast<float4*>(pp.pool_raw + po) = make_float4(yb[q][0], yb[q][1], yb[q][2], yb[q][3]);
                } else {
                    *reinterpret_cast<float4*>(pp.pool_raw + po) = make_float4(yb[q][0], yb[q][1], yb[q][2], yb[q][3]);
                }
            }
        }
        if (want_stats) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float a1 = s1[q], a2 = s2[q];
                a1 += __shfl_xor(a1, 16, 64);
                a1 += __shfl_xor(a1, 32, 64);
                a2 += __shfl_xor(a2, 16, 64);
                a2 += __shfl_xor(a2, 32, 64);
                if (fk == 0) {
                    const int slot = ((T * 4 + wave) * 4 + q) * 16 + fr;
                    sred[slot * 2 + 0] = a1;
                    sred[slot * 2 + 1] = a2;
                }
            }
        }
    };
    tile_body(std::integral_constant<int, 0>{});
    if constexpr (NT > 1) tile_body(std::integral_constant<int, 1>{});
    if constexpr (NT > 2) tile_body(std::integral_constant<int, 2>{});

    // hcq_stats_flush of hcq_conv.h with this kernel's slot index, written out: through the shared function five of the
    // eight y-writing instantiations allocate one or two registers more or fewer
    if (want_stats) {
        __syncthreads();
        float* rep = p.stats[0] + (size_t)(blockIdx.x % SELD_STATS_REPLICAS) * 2 * p.Cdst;
        for (int e = tid; e < NT * 4 * 16; e += 256) {
            const int fr_ = e & 15, q = (e >> 4) & 3, t = e >> 6;
            const int g_ = fr_ >> 3;
            const int ob0 = p.t.tile_ob[t][g_];
            if (ob0 < 0) continue;
            const int chn = (p.t.tile_half[t][g_] * 4 + q) * p.OB + ob0 + (fr_ & 7);
            float a1 = 0.f, a2 = 0.f;
#pragma unroll
            for (int wv = 0; wv < 4; ++wv) {
                const int slot = ((t * 4 + wv) * 4 + q) * 16 + fr_;
                a1 += sred[slot * 2 + 0];
                a2 += sred[slot * 2 + 1];
            }
            atomicAdd(rep + chn, a1);
            atomicAdd(rep + p.Cdst + chn, a2);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
// the first layers' kernels: 3x3 with one or two block channels, no mixed-tile workgroups
template <int I, int V> constexpr bool hcq_is_first() { return HCQ_INST[I].KH == 3 && HCQ_INST[I].IBC <= 2 && !HCQ_TILEV[V].MX; }

template <int I, int V>
struct HcqLaunchFirst {
    static int run(const HcqPlan& pl, hipStream_t st) {
        constexpr HcqTileV T = HCQ_TILEV[V];
        if constexpr (hcq_is_first<I, V>())
            return hcq_launch_kernel(hcq_first_kernel<HCQ_INST[I].IBC, T.NT1, T.NT2, T.NR, HCQ_FIRST_R>, pl, st, pl.kp);
        return SELD_EUNSUPPORTED;
    }
};

// fin: BatchNorm + ReLU + Dropout applied to the window value; else y is written (with statistics) or not at all
template <int I, int V>
struct HcqLaunchPool {
    static int run(const HcqPlan& pl, const HcqPoolP& pp, bool fin, hipStream_t st) {
        constexpr HcqTileV T = HCQ_TILEV[V];
        if constexpr (hcq_is_first<I, V>()) {
            constexpr int IBC = HCQ_INST[I].IBC;
            if (fin) return hcq_launch_kernel(hcq_first_pool_kernel<IBC, T.NT1, T.NT2, T.NR, HCQ_FIRST_R, false, true>, pl, st, pl.kp, pp);
            if (pl.kp.dst[0]) return hcq_launch_kernel(hcq_first_pool_kernel<IBC, T.NT1, T.NT2, T.NR, HCQ_FIRST_R, true>, pl, st, pl.kp, pp);
            return hcq_launch_kernel(hcq_first_pool_kernel<IBC, T.NT1, T.NT2, T.NR, HCQ_FIRST_R, false>, pl, st, pl.kp, pp);
        }
        return SELD_EUNSUPPORTED;
    }
};

int hcq_launch_first(const HcqPlan& pl, hipStream_t st) {
    SELD_HCQ_DISPATCH(HcqLaunchFirst, pl, st)
    return SELD_EUNSUPPORTED;
}

}  // namespace seld

using namespace seld;

/* conv -> [BatchNorm2d -> ReLU ->] MaxPool2d(8, 1) for the network's first layer (model.py:273-281), pooling decision
 * inside the convolution (hcq_first_pool_kernel): writes y (nullable: not written, and then no statistics either -- the
 * seld_first_stage_* path), the BatchNorm statistics (want_stats), and per pooling window
 * the raw value at the row that will be the maximum after BatchNorm + ReLU (by the sign of gamma) and that row.
 * wpack: seld_hcq_pack(desc, mode 2).  Follow with seld_bn_finalize_ex and seld_bn_pool_finish. */
static int hcq_first_pool_impl(const seld_conv_desc* d, const float* x, const float* wpack, const float* bias,
                               int32_t want_stats, float* y, float* stats, const HcqPoolP& pp, bool fin, void* stream) {
    HcqPlan pl = hcq_plan(d, 2, 1);
    if (!pl.ok) return SELD_EUNSUPPORTED;
    pl.kp.src = x; pl.kp.src2 = nullptr; pl.kp.wpack = wpack;
    pl.kp.dst[0] = y; pl.kp.bias[0] = bias; pl.kp.epilogue[0] = want_stats ? SELD_EPI_STATS : 0; pl.kp.stats[0] = stats;
    SELD_HCQ_DISPATCH(HcqLaunchPool, pl, pp, fin, (hipStream_t)stream)
    return SELD_EUNSUPPORTED;
}

extern "C" int seld_hcq_first_pool(const seld_conv_desc* d, const float* x, const float* wpack, const float* bias,
                                   const float* gamma, int32_t want_stats, float* y, float* stats, float* pool_raw,
                                   uint8_t* idx, void* stream) {
    if (hc_validate(d) != SELD_OK || !x || !wpack || !gamma || !pool_raw || !idx || (want_stats && (!stats || !y))) return SELD_EINVAL;
    const HcqPoolP pp{gamma, pool_raw, idx, nullptr, nullptr, nullptr, nullptr, DropP{0.f, 1.f, 0, 0, nullptr}};
    return hcq_first_pool_impl(d, x, wpack, bias, want_stats, y, stats, pp, false, stream);
}

extern "C" int seld_hcq_first_pool_bn(const seld_conv_desc* d, const float* x, const float* wpack, const float* bias,
                                      const float* gamma, const float* beta, const float* mean, const float* invstd,
                                      float drop_p, uint64_t seed, uint64_t offset, const uint64_t* state, float* pool_raw,
                                      uint8_t* idx, float* out, void* stream) {
    if (hc_validate(d) != SELD_OK || !x || !wpack || !gamma || !beta || !mean || !invstd || !pool_raw || !idx || !out ||
        drop_p < 0.f || drop_p >= 1.f)
        return SELD_EINVAL;
    const HcqPoolP pp{gamma, pool_raw, idx, beta, mean, invstd, out, DropP{drop_p, 1.0f / (1.0f - drop_p), seed, offset, state}};
    return hcq_first_pool_impl(d, x, wpack, bias, 0, nullptr, nullptr, pp, true, stream);
}
