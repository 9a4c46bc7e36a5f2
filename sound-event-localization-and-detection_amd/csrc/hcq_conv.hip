// Quaternion / dual-quaternion convolution with the 8-multiplication Hamilton product (gfx950), forward and data
// gradient of the 1-D layers (1x3 dilated, 1x1) and the 3x3 layers.
//
// In this file: hcq_conv_kernel; the kernels that pack the weight forms (hcq_pack_kernel for one layer, hcq_pack_flat_kernel
// for every registered layer in one launch); hcq_plan, which decides kernel, tile program, ring, grid and LDS for a
// (descriptor, mode, pair count); the seld_hcq_* entry points.  The row-walking kernels of the first layers and the two
// pooling entry points are in hcq_first.hip; launch arguments, instantiation table, dispatch macros and the device
// pieces that more than one kernel uses in hcq_conv.h.
//
// A Hamilton product w (x) x costs 16 real sub-products when it is evaluated as the 4 x 4 block matrix the reference
// assembles (quaternion_ops.py:131-135).  It is a bilinear map of rank 8: eight products P_m = F_m(a) G_m(b) of sums of
// two components, recombined into the four components of c (the forms, the recombination and the proof that they are
// the Hamilton product: hcq_forms.h)
//
// (a = weight components r,i,j,k; b = input components; c = output components; the a's always stand on the left, so
// the identities hold for matrix-valued components, i.e. for convolutions).  The convolution therefore splits into 8
// INDEPENDENT real GEMMs  P_m = F_m(W) * G_m(X)  of one quarter of the K extent each -- half the MFMA work of the block
// matrix -- plus sums of two components on the way in and a signed sum of the eight accumulators on the way out.
// In fp32 the result differs from the 16-product evaluation by rounding only (measured against fp64 on the TCN layer:
// 2.5e-7 of max|y| against 1.8e-7 for the 16-product form).  The dual quaternion [[Q, 0], [Q2, Q]] is three such
// products, y_p = Q x_p,  y_d = Q2 x_p + Q x_d: 24 sub-products instead of 48.
//
// Kernel structure (one workgroup = 4 waves = 64 positions x one channel tile, 2 or 3 workgroups per CU):
//   * the weight forms F_m are precomputed ONCE per step by hcq_pack_kernel, already in MFMA B-fragment order
//     ([chunk][range][k-group pair][m][lane][tile][2]), so a workgroup's fragments are one linear stream.  The workgroup
//     copies it unit by unit (the 8 forms of a pair of k-groups, or 4 of them) into a ring of two LDS slots with LDS-DMA
//     and its four waves read their fragments there, form by form, two forms ahead of the MFMAs: a fragment passes the
//     CU's vector L1 once per workgroup, not once per wave, and a wave holds 3 forms in registers, not 8;
//   * the input is staged RAW (no im2col), also by LDS-DMA: per K chunk of IBC block channels the 4 / 8 component rows of
//     the tile plus their halo, [component][channel][64 + 2*dpad] floats, double-buffered; the taps are offsets into rows;
//   * per pair of k-groups a lane reads its 2 x 4 component values, forms the 2 x 8 sums G_m (16 VALU) and issues, form
//     by form, tiles MFMAs (v_mfma_f32_16x16x4_f32) for the even and then the odd k-group into accumulators [tile][m];
//   * one barrier per unit (see the K loop for the wait counts); the next chunk's input is requested at a chunk's first
//     unit and has two units of MFMAs to arrive in;
//   * two K ranges for the dual quaternion: range 0 reads the source half every output needs, range 1 the half only
//     one half of the outputs needs (the structural zero block is never touched);
//   * epilogue: the signed sums above, bias / addend / BatchNorm statistics, 16-byte stores.
// Registers / LDS per workgroup (input buffers + ring) / workgroups per CU that LDS allows, at the step's shapes:
//   cnn.1 / cnn.2  <3,3,4,1,2,2,7>      188 VGPRs (221 before the ring)   55 296 + 24 576 B   2
//   TCN 1x3 halo 4 <1,3,8,1,1,2,5>      113 (152); mixed tiles 127 (165)  36 864 + 16 384     3
//   TCN 1x3 halo 8, forward             113                               40 960 +  8 192     3   (half-pair slots)
//   TCN 1x3 halo 8, data gradient       127                               40 960 + 16 384     2   (mixed tiles: see hcq_plan)
//   TCN 1x3 halo 16, forward            global loads (GF): 49 152 B of input leave no room for a ring at 3 per CU
//   TCN 1x1 pair   <1,1,16,1,2,2,8>     168 (198)                         65 536 + 12 288     2   (half-pair slots)
// No instantiation spills.
#include "hcq_conv.h"

// Phase ablation for timing experiments only (tools/hcq_ablate.sh builds variants into tools/_bin; results are WRONG with
// any bit set): 1 = weight fragments requested once (every unit reads slot 0), 2 = LDS operand reads + sums once,
// 4 = input staged twice only, 8 = no barriers.  The shipped library is built with 0.
// Readings on cnn.1 (forward / data gradient, us).  With per-wave global fragment loads (the kernel before the ring, now
// the GF form): as shipped 774 / 732; 1: 636 / 591; 4: 718 / 668; 8: no change; 1+2+4: 550 / 517 (the MFMA floor is 481).
// The fragment loads were the largest term, and it was not their bytes, their request count or their latency window
// that cost: loading the 4 raw components per (pair, tile) and forming the 8 sums in registers (half the bytes and
// requests, two register stages = a whole pair of k-groups ahead) ran 773 / 745, with three-wave occupancy lost on the
// TCN layers (177 VGPRs) -- and again 757 against 701 once both versions had their requests pinned (HCQ_PIN), for the
// three-tile shapes only; raised wave priority (s_setprio 1) around each k-group's MFMAs 786 / 786; rotating the chunk
// order per workgroup (so that workgroups in step do not ask the L2 for the same lines) 751 / 723 against 752 / 722;
// staging the input from cache-resident addresses 712 against 723.  What cost was WHO asked: four waves fetching the same
// fragments through one L1 (0.78 tag accesses per CU clock).  With the ring (tools/hcq_check.py, medians of three,
// same session): cnn.1 728 / 660 against 747 / 686, L1 accesses per CU clock 0.16 against 0.78, MFMA busy 66.2 % against 65.0 %
// (profiles/hcq_fragment_ring_counters.txt, profiles/hcq_fragment_ring_shapes.md).  The ablation variants have not been
// re-measured with the ring.
#ifndef HCQ_DBG
#define HCQ_DBG 0
#endif
#ifndef HCQ_PIN
#define HCQ_PIN 1
#endif

namespace seld {

// KH x KW taps (1x1, 1x3, 3x3), IBC block channels per K chunk, NT1 tiles active in range 0 only + NT2 tiles active
// in both ranges (NR = 1: quaternion, one range), XI staging items per thread.
// The channel tile p.mix_ytile (dual quaternion with 24 block channels, split layout) runs the same program with other
// descriptors: its range-0-only tile is padding, its both-range tile is descriptor slot 2 (8 channels of each half).
// MX: the launch has mixed-tile workgroups, whose copy of the K loop leaves the padding slots out (a second copy of the
// loop costs registers -- 186 instead of 160 for the TCN 1x3 shape -- so launches without such workgroups keep MX = false).
// GF: the shapes hcq_plan keeps off the fragment ring (quaternion 1-D layers; 1-D shapes whose LDS has no room for it):
// every wave loads its own fragments from global memory, as all launches did before the ring.
template <int KH, int KW, int IBC, int NT1, int NT2, int NR, int XI, bool MX = false, bool GF = false>
__global__ __launch_bounds__(256, 2) void hcq_conv_kernel(const HcqP p) {
    constexpr int TAPS = KH * KW;
    constexpr int NT = NT1 + NT2;
    constexpr int KQ = IBC * TAPS;
    constexpr int NG = (KQ + 3) / 4;                  // the first layers (1 or 2 block channels x 9 taps) pad the last k-group:
                                                      // packed weights are zero there, the lane re-reads k = 0
    constexpr int NPAIR = (NG + 1) / 2;
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fk = lane >> 4;
    const int A = p.A;
    const int ROWS = A * IBC * KH;                    // staged rows per chunk
    const int wext = p.wext, qw = wext >> 2;
    const int buf_floats = ROWS * wext;

    // ---- tile position (32-bit arithmetic throughout: the host checked that both tensors are below 4 GB) ------------
    const unsigned tiles_per_row = (unsigned)p.W >> 6;    // 64 consecutive positions inside ONE row (W % 64 == 0)
    const unsigned bx = hcq_xcd_block();
    const unsigned row_g = bx / tiles_per_row;            // n * Himg + h
    const int w0 = (int)(bx - row_g * tiles_per_row) * 64;
    const int n_img = (int)(row_g / (unsigned)p.Himg);
    const int h0 = (int)row_g - n_img * p.Himg;
    const int yt = blockIdx.y;                        // channel tile over all weight sets
    const int set = yt >= p.ytiles ? 1 : 0;           // at most two weight sets
    const int ytile = yt - set * p.ytiles;
    const bool mix_wg = ytile == p.mix_ytile;         // workgroup-uniform

    // ---- staging items: (row, quad) of the raw image of a chunk, everything but the chunk advance is invariant ----
    const unsigned S = (unsigned)(p.Himg * p.W);
    const unsigned src_bytes = (unsigned)p.N * (unsigned)p.Csrc * S * 4u;
    const unsigned OOB = 0xFFFFFFF0u;
    unsigned xoff[XI];
    int xlds[XI];
    const unsigned xadv = (unsigned)IBC * S * 4u;
    const int total_items = ROWS * qw;
    {
        // item f = tid + 256 i  ->  (row, quad) = (f / qw, f % qw): one division, then increments
        int row = small_div_h(tid, 1.0f / (float)qw);
        int quad = tid - row * qw;
        const int drow = 256 / qw, dquad = 256 - drow * qw;       // wave-uniform
        const unsigned img_base = (unsigned)n_img * (unsigned)p.Csrc * S;
#pragma unroll
        for (int i = 0; i < XI; ++i) {
            const bool in = tid + 256 * i < total_items;
            // row = (comp * IBC + ibl) * KH + kh, all divisors compile-time
            const int kh = row % KH;
            const int ci = row / KH;
            const int comp = ci / IBC;
            const int ibl = ci - comp * IBC;
            const int hh = h0 + (kh - (KH - 1) / 2);
            const int ww = w0 - p.dpad + 4 * quad;
            const bool ok = in && (unsigned)hh < (unsigned)p.Himg && (unsigned)ww < (unsigned)p.W;
            const unsigned e = img_base + ((unsigned)(comp * p.IB + ibl) * (unsigned)p.Himg + (unsigned)hh) * (unsigned)p.W + (unsigned)ww;
            xoff[i] = ok ? e * 4u : OOB;
            xlds[i] = in ? (row * qw + quad) * 4 : -1;     // float index of the quad in the LDS image; -1: no store
            row += drow;
            quad += dquad;
            if (quad >= qw) { quad -= qw; ++row; }
        }
    }
    // Input chunks go global -> LDS directly (buffer_load ... lds): the LDS image is linear in the item index (item f at byte
    // 16 f), so instruction i of wave w fills the contiguous KiB at 16 (256 i + 64 w); no staging registers (28 of them for
    // the 3x3 layers), no ds_write.  load_x(buf) requests the next chunk into `buf`; store_x waits for the wave's requests.
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)lds;
    int4h xrs = hcq_rsrc(p.src, src_bytes);
    int xchunk = 0;                                    // chunks requested so far
    int xbuf = 0;                                      // buffer the next request fills
    auto load_x = [&]() __attribute__((always_inline)) {
        if (xchunk == p.nch) {                         // second source of a pair: same offsets, other tensor
            xrs = hcq_rsrc(p.src2, src_bytes);
#pragma unroll
            for (int i = 0; i < XI; ++i) xoff[i] = xoff[i] == OOB ? OOB : xoff[i] - (unsigned)p.nch * xadv;
        }
        ++xchunk;
        const unsigned base = lds0 + (unsigned)xbuf * (unsigned)buf_floats * 4u + 1024u * (unsigned)wave;
#pragma unroll
        for (int i = 0; i < XI; ++i) {
            if (xlds[i] >= 0) hcq_dma16(base + 4096u * (unsigned)i, xoff[i], xrs);
            xoff[i] = xoff[i] == OOB ? OOB : xoff[i] + xadv;
        }
        xbuf ^= 1;
    };
    auto store_x = [&](int) __attribute__((always_inline)) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); };

    // ---- A-operand addresses: k-group g, this lane's k = 4g + fk -> (ibl, kh, kw); component stride = IBC*KH*wext ----
    int aoff[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int kq = (4 * g + fk) < KQ ? 4 * g + fk : 0;
        const int ibl = kq / TAPS;
        const int tap = kq - ibl * TAPS;
        const int kh = tap / KW;
        const int kw = tap - kh * KW;
        aoff[g] = (ibl * KH + kh) * wext + p.dpad + wave * 16 + fr + (kw - (KW - 1) / 2) * p.dil;
    }
    const int comp_stride = IBC * KH * wext;

    // ---- weight fragments ------------------------------------------------------------------------------------------
    const float* wbase = p.wpack + (long long)set * p.t.set_stride + (long long)ytile * p.t.ytile_stride;
    const long long chunk_stride = p.t.range_stride[0] + (NR > 1 ? p.t.range_stride[1] : 0);

    floatx4 acc[NT][8];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int m = 0; m < 8; ++m) acc[t][m] = (floatx4){0.f, 0.f, 0.f, 0.f};

    // ---- one K chunk = range 0's NG k-groups, then range 1's.  Software pipeline, forced with scheduling barriers
    // (left alone, the compiler sinks every fragment load to just before its MFMA and waits for it there: 43 % MFMA busy):
    //   * weight fragments come in pairs of k-groups, one register pair per form; a form's registers are re-requested
    //     for the next pair (or the next chunk's first pair) right after their last MFMA, so every request has the other
    //     seven forms' MFMAs and the next group's first ones in front of its use -- one stage instead of two keeps the
    //     kernel at 3 waves per SIMD;
    //   * the raw component values of k-group g+1 are read from LDS at the start of group g and turned into the 8 sums
    //     under the MFMAs of group g, so no VALU result feeds the very next MFMA.
    float2 bfr[8][NT];                                       // ONE stage: form m's pair is re-requested right after its last use
    float gm[2][8];
    float raw[4];
    constexpr int NPC = NR * NPAIR;                          // fragment pairs per chunk

    bool dbg_started = false;
    // T0: first tile that is loaded (a mixed-tile workgroup's range-0-only slots are padding: neither loaded nor multiplied)
    auto load_b1 = [&](const float* blk, int j, int m, auto ntrc, auto t0c) __attribute__((always_inline)) {
        constexpr int NTR = decltype(ntrc)::value, T0 = decltype(t0c)::value;
        if ((HCQ_DBG & 1) && dbg_started) return;
        const float* q = blk + ((long long)(j * 8 + m) * 64 + lane) * (2 * NTR);
#pragma unroll
        for (int t = T0; t < NTR; ++t) bfr[m][t] = *reinterpret_cast<const float2*>(q + 2 * t);
    };
    auto read_raw = [&](const float* xs, int g) __attribute__((always_inline)) {
        if ((HCQ_DBG & 2) && dbg_started) return;
#pragma unroll
        for (int q = 0; q < 4; ++q) raw[q] = xs[aoff[g] + q * comp_stride];
    };
    using I0 = std::integral_constant<int, 0>;
    using INT = std::integral_constant<int, NT>;
    using INT1 = std::integral_constant<int, NT1>;
    using INT2 = std::integral_constant<int, NT2>;

    // ---- K loop ------------------------------------------------------------------------------------------------
    // MIX: the workgroup of the mixed 8 + 8 tile (descriptor slot 2 in accumulator slot NT1).  Its range-0-only slots are
    // padding; round 2 ran the same program on zero weights for them (a third of such a workgroup's MFMAs), now they are
    // compiled out of its copy of the loop.
    const int nchunks = p.nch * p.nsrc;
    auto kloop = [&](auto mixc) __attribute__((always_inline)) {
    constexpr bool MIX = decltype(mixc)::value;
    using IT0 = std::integral_constant<int, MIX ? NT1 : 0>;
    load_x();
    store_x(0);
#pragma unroll
    for (int m = 0; m < 8; ++m) load_b1(wbase, 0, m, INT{}, IT0{});
    __syncthreads();
    for (int ch = 0; ch < nchunks; ++ch) {
        const int buf = ch & 1;
        if (ch + 1 < nchunks && !(HCQ_DBG & 4)) load_x();
        const float* xb = lds + buf * buf_floats;
        const float* wc = wbase + (long long)ch * chunk_stride;
        const bool more = ch + 1 < nchunks;
        const float* wn = wc + chunk_stride;
        const float* xs0 = xb + p.t.half_src[0] * 4 * comp_stride;
        const float* xs1 = xb + p.t.half_src[1] * 4 * comp_stride;
        read_raw(xs0, 0);
        if (!(HCQ_DBG & 2) || !dbg_started) hcq_xforms(raw, gm[0]);
        if ((HCQ_DBG & 2) && !dbg_started) hcq_xforms(raw, gm[1]);
        dbg_started = true;
#pragma unroll
        for (int s = 0; s < NR * NG; ++s) {                   // k-groups of the chunk, both ranges
            const int r = s / NG, g = s - r * NG;
            const int pc = r * NPAIR + g / 2;                // fragment pair of this group within the chunk
            const int gst = s & 1;
            const bool last = s + 1 == NR * NG;
            const bool pair_ends = (g & 1) == 1 || g + 1 == NG;   // last k-group that uses the current fragments
            if (!last) {
                const int rn = (s + 1) / NG, gn = (s + 1) - rn * NG;
                read_raw(rn == 0 ? xs0 : xs1, gn);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                if (r == 0) {
#pragma unroll
                    for (int t = MIX ? NT1 : 0; t < NT; ++t)
                        acc[t][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(gm[gst][m], (g & 1) ? bfr[m][t].y : bfr[m][t].x,
                                                                          acc[t][m], 0, 0, 0);
                } else {
#pragma unroll
                    for (int t = 0; t < NT2; ++t)
                        acc[NT1 + t][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(gm[gst][m], (g & 1) ? bfr[m][t].y : bfr[m][t].x,
                                                                                acc[NT1 + t][m], 0, 0, 0);
                }
                if (pair_ends) {                              // form m's fragments are free: request the next pair's
                    const int pn = pc + 1;
                    if (pn < NPC) {
                        const int rn = pn / NPAIR, jn = pn - rn * NPAIR;
                        if (rn == 0) load_b1(wc, jn, m, INT{}, IT0{});
                        else load_b1(wc + p.t.range_stride[0], jn, m, INT2{}, I0{});
                    } else if (more) {
                        load_b1(wn, 0, m, INT{}, IT0{});
                    }
                    // keep the request HERE: between two scheduling barriers the compiler moves loads towards their use
                    // (register pressure), i.e. to the end of this k-group -- a few MFMAs ahead of the wait instead of
                    // seven forms
                    if (HCQ_PIN) __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (!last && !(HCQ_DBG & 2)) hcq_xforms(raw, gm[gst ^ 1]);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (ch + 1 < nchunks && !(HCQ_DBG & 4)) store_x(buf ^ 1);
        if (!(HCQ_DBG & 8)) __syncthreads();
    }
    };

    // ---- K loop with the fragment ring ------------------------------------------------------------------------------
    // The packed fragments of a workgroup are ONE linear stream: [chunk][range][pair][form m][lane][tile][2].  It is cut
    // into units of 8 forms (a pair of k-groups: 4 KB x tiles of the range) or 4 forms (p.half_slots); unit u is copied by
    // the whole workgroup into ring slot u & 1 with LDS-DMA (a linear copy: instruction i of wave w moves the KiB 4 i + w),
    // so a fragment passes the vector L1 once per workgroup instead of once per wave.
    //   open(u):   s_waitcnt vmcnt -- this wave's copy of unit u has landed;  s_waitcnt lgkmcnt(0) + s_barrier -- so has
    //              everybody's, and everybody has finished reading unit u - 1 (and, at a chunk's first unit, the previous
    //              chunk's input buffer);
    //   then:      request unit u + 1 into the slot of unit u - 1; at a chunk's first unit request the NEXT chunk's input
    //              behind it; read the 2 x 4 raw component values of the pair, form the sums; per form read the lane's
    //              2 x tiles floats from the slot two forms ahead of their MFMAs (three register stages instead of the
    //              eight of the global-load loop).
    // vmcnt retires in order.  Requests of a wave between two opens:   open(first unit of chunk): F(u+1), X(next chunk) [XI]
    //                                                                  open(second unit):          F(u+2)
    // so the second unit's open waits with vmcnt(XI) (only F(u+1) has to be there, the XI input requests behind it stay in
    // flight) and every other open with vmcnt(0): the input of the next chunk has two units of MFMAs to arrive in.  A wave
    // whose last staging instruction has no lane to serve (its count is not XI) waits with vmcnt(0) there, too.
    // An accumulator sees its k-groups in the order of the global-load loop (a pair's even group, then its odd one), so the
    // results are the same bits.
    auto kring = [&](auto mixc) __attribute__((always_inline)) {
    constexpr bool MIX = decltype(mixc)::value;
    const bool half = p.half_slots != 0;                        // workgroup-uniform
    const unsigned tile_bytes = half ? 2048u : 4096u;           // one tile's share of a unit
    const unsigned slot_bytes = tile_bytes * NT;
    const unsigned ring0 = lds0 + (unsigned)p.ring_off;
    const float* const ringf = lds + (p.ring_off >> 2);
    const int4h frs = hcq_rsrc(wbase, (unsigned)p.t.ytile_stride * 4u);     // this channel tile's fragments, all chunks and sources
    unsigned foff = 1024u * (unsigned)wave + 16u * (unsigned)lane;        // of the next unit to request
    unsigned fslot = 0;                                          // slot the next request fills
    unsigned rslot = 0;                                          // slot of the unit being read
    bool freq = false;
    const bool xfull = 256 * (XI - 1) + 64 * wave < total_items; // this wave issues all XI staging instructions of a chunk
    auto load_f = [&](auto ntrc) __attribute__((always_inline)) {
        constexpr int NTRn = decltype(ntrc)::value;
        const unsigned nbytes = tile_bytes * NTRn;
        if (!((HCQ_DBG & 1) && freq)) {
            const unsigned dst = ring0 + fslot * slot_bytes + 1024u * (unsigned)wave;
#pragma unroll
            for (int i = 0; i < NTRn; ++i)
                if (4096u * i + 1024u * (unsigned)wave < nbytes) hcq_dma16(dst + 4096u * i, foff + 4096u * i, frs);   // wave-uniform
        }
        freq = true;
        foff += nbytes;
        fslot ^= 1u;
    };
    // counted: XI younger requests (the next chunk's input) may stay in flight
    auto open_unit = [&](bool counted) __attribute__((always_inline)) {
        if (counted) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(XI) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (HCQ_DBG & 8) return;
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    };
    float ga[8], gb[8];
    float2 fb[3][NT];
    load_x();                                                    // chunk 0
    load_f(INT{});                                               // unit 0
    bool dbg_raw = false;
    for (int ch = 0; ch < nchunks; ++ch) {
        const bool more = ch + 1 < nchunks;
        const float* xb = lds + (ch & 1) * buf_floats;
        const float* xs0 = xb + p.t.half_src[0] * 4 * comp_stride;
        const float* xs1 = xb + p.t.half_src[1] * 4 * comp_stride;
        bool xreq = false;                                       // the next chunk's input was requested at this chunk's first open
#pragma unroll
        for (int pc = 0; pc < NPC; ++pc) {
            const int r = pc / NPAIR, j = pc - r * NPAIR;
            const int g0 = 2 * j;
            const bool two = g0 + 1 < NG;                        // (the last pair of an odd NG holds one k-group)
            const int ntr = r == 0 ? NT : NT2;
            const int t0 = (r == 0 && MIX) ? NT1 : 0;
            const int ab = r == 0 ? 0 : NT1;                     // accumulator slot of the range's first tile
            // the unit after this pair's last one: the next pair's first (next range, next chunk)
            auto request_next_pair = [&]() __attribute__((always_inline)) {
                if (pc + 1 < NPC) {
                    if ((pc + 1) / NPAIR == 0) load_f(INT{});
                    else load_f(INT2{});
                } else if (more) {
                    load_f(INT{});
                }
            };
            // ---- open the pair's first unit; second unit of the chunk when pc == 1 and slots hold whole pairs
            open_unit(pc == 1 && !half && xreq && xfull);        // vmcnt: F(this unit) | X x XI, or everything
            if (half) {
                if (r == 0) load_f(INT{});
                else load_f(INT2{});
            } else {
                request_next_pair();
            }
            if (pc == 0 && more && !((HCQ_DBG & 4) && ch > 0)) { load_x(); xreq = true; }
            const float* fsl = ringf + rslot * (slot_bytes >> 2);
            auto read_form = [&](int idx, int st) __attribute__((always_inline)) {
                const float2* q = reinterpret_cast<const float2*>(fsl) + (idx * 64 + lane) * ntr;
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (t >= t0 && t < ntr) fb[st][t] = q[t];
            };
            read_form(0, 0);
            read_form(1, 1);
            if (!((HCQ_DBG & 2) && dbg_raw)) {
                float ra[4], rb[4];
                const float* xs = r == 0 ? xs0 : xs1;
#pragma unroll
                for (int q = 0; q < 4; ++q) ra[q] = xs[aoff[g0] + q * comp_stride];
                if (two) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) rb[q] = xs[aoff[two ? g0 + 1 : g0] + q * comp_stride];
                }
                hcq_xforms(ra, ga);
                if (two) hcq_xforms(rb, gb);
                dbg_raw = true;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                if (m == 4 && half) {
                    // ---- the pair's second unit (4-form slots): second unit of the chunk when pc == 0
                    open_unit(pc == 0 && xreq && xfull);         // vmcnt: F(this unit) | X x XI, or everything
                    request_next_pair();
                    rslot ^= 1u;
                    fsl = ringf + rslot * (slot_bytes >> 2);
                    read_form(0, 4 % 3);
                    read_form(1, 5 % 3);
                }
                if (m + 2 < 8) {
                    if (m + 2 < 4 || m >= 4) read_form(half ? (m + 2) & 3 : m + 2, (m + 2) % 3);
                    else if (!half) read_form(m + 2, (m + 2) % 3);      // forms 4, 5 of a whole-pair slot
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (t >= t0 && t < ntr)
                        acc[ab + t][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[m], fb[m % 3][t].x, acc[ab + t][m], 0, 0, 0);
                if (two) {
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        if (t >= t0 && t < ntr)
                            acc[ab + t][m] = __builtin_amdgcn_mfma_f32_16x16x4f32(gb[m], fb[m % 3][t].y, acc[ab + t][m], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            rslot ^= 1u;
            if (HCQ_DBG & 1) rslot = 0;
        }
    }
    // the statistics scratch of the epilogue overlays the staging area: not before everybody's last reads
    if (p.epilogue[set] & SELD_EPI_STATS) __syncthreads();
    };
    if constexpr (MX) {
        static_assert(NR == 2 && NT1 == 1 && NT2 == 1, "the only layout with mixed-tile workgroups");
        if constexpr (GF) {
            if (mix_wg) kloop(std::true_type{});
            else kloop(std::false_type{});
        } else {
            if (mix_wg) kring(std::true_type{});
            else kring(std::false_type{});
        }
    } else {
        if constexpr (GF) kloop(std::false_type{});
        else kring(std::false_type{});
    }

    // ---- epilogue ------------------------------------------------------------------------------------------------
    float* const dst = p.dst[set];
    const float* const bias = p.bias[set];
    const float* const addend = p.addend[set];
    const int epi = p.epilogue[set];
    const int grp = fr >> 3;
    const unsigned pos_off = (unsigned)h0 * (unsigned)p.W + (unsigned)(w0 + wave * 16 + fk * 4);
    const unsigned img_off = (unsigned)n_img * (unsigned)p.Cdst * S;
    float* redbuf = lds;                       // the K loop is over (last barrier passed): staging buffers are free
    // PLAIN: no bias / addend / accumulate / statistics (every data gradient, the plain forward): stores only
    auto epilogue = [&](auto plainc) __attribute__((always_inline)) {
        constexpr bool PLAIN = decltype(plainc)::value;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            // a mixed-tile workgroup: accumulator slot NT1 is descriptor slot 2, the other slots are padding
            // (hcq_lane_channel's decode in a spelling of its own: through the helper 11 instantiations allocate 1 to 6
            //  registers fewer and five of them run at another occupancy -- DESIGN.md)
            const int ds = mix_wg ? 2 : t;
            const int ob0 = (mix_wg && t != NT1) ? -1 : p.t.tile_ob[ds][grp];
            const int half = p.t.tile_half[ds][grp];
            const bool chok = ob0 >= 0;
            const int ob = (chok ? ob0 : 0) + (mix_wg ? 0 : ytile * p.t.ob_step) + (fr & 7);
            floatx4 c[4];
            hcq_recombine4(acc[t], c);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int chn = (half * 4 + q) * p.OB + ob;           // component-major channel index
                const unsigned off = img_off + (unsigned)chn * S + pos_off;
                if (PLAIN) {
                    if (chok) *reinterpret_cast<float4*>(dst + off) = make_float4(c[q][0], c[q][1], c[q][2], c[q][3]);
                    continue;
                }
                float s1 = 0.f, s2 = 0.f;
                if (chok) {
                    const float bv = bias ? bias[chn] : 0.f;
                    float4 o = make_float4(c[q][0] + bv, c[q][1] + bv, c[q][2] + bv, c[q][3] + bv);
                    if (epi & SELD_EPI_ADD) {
                        const float4 ad = *reinterpret_cast<const float4*>(addend + off);
                        o.x += ad.x; o.y += ad.y; o.z += ad.z; o.w += ad.w;
                    }
                    if (epi & SELD_EPI_ACCUMULATE) {
                        const float4 old = *reinterpret_cast<const float4*>(dst + off);
                        o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w;
                    }
                    *reinterpret_cast<float4*>(dst + off) = o;
                    s1 = o.x + o.y + o.z + o.w;
                    s2 = o.x * o.x + o.y * o.y + o.z * o.z + o.w * o.w;
                }
                if (epi & SELD_EPI_STATS) {
                    s1 += __shfl_xor(s1, 16, 64);
                    s1 += __shfl_xor(s1, 32, 64);
                    s2 += __shfl_xor(s2, 16, 64);
                    s2 += __shfl_xor(s2, 32, 64);
                    if (fk == 0) {
                        const int slot = ((wave * NT + t) * 4 + q) * 16 + fr;
                        redbuf[slot * 2 + 0] = s1;
                        redbuf[slot * 2 + 1] = s2;
                    }
                }
            }
        }
    };
    if (epi == 0 && !bias) epilogue(std::true_type{});
    else epilogue(std::false_type{});
    if (epi & SELD_EPI_STATS)
        hcq_stats_flush<NT, 1>(p, set, tid, mix_wg ? NT1 : -1, mix_wg ? 0 : ytile * p.t.ob_step, redbuf, 1,
                               [](int wv, int, int t, int q, int fr_) __attribute__((always_inline)) {
                                   return (((wv * NT + t) * 4 + q) * 16 + fr_) * 2;
                               });
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight forms in fragment order.  One thread per packed float.
//   mode 0 (forward):        dst block channel = conv output block channel, K runs over (conv input block channel, tap)
//   mode 1 (data gradient):  dst = conv INPUT block channel, K over (conv output block channel, flipped tap), conjugate
// Layout: [weight set (forward pairs)] x { regular channel tiles [ytile][source (gradient pairs)][chunk][range][pair]
// [m][lane][tile][2 groups], the mixed channel tile (if any) last, same layout }.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float hcq_pack_value(const HcqPackP& p, long long idx) {
    // 32-bit index arithmetic (the host keeps every buffer below 2^31 floats): the 64-bit divisions this decode started
    // with were most of the kernel's 60 us
    const int NT = p.t.NT1 + p.t.NT2;
    const unsigned set_stride = (unsigned)p.t.set_stride, ytile_stride = (unsigned)p.t.ytile_stride;
    const unsigned set = (unsigned)idx / set_stride;
    unsigned r0 = (unsigned)idx - set * set_stride;
    const int ytile = (int)(r0 / ytile_stride);
    r0 -= (unsigned)ytile * ytile_stride;
    const bool mix = p.t.mix && ytile == p.t.nreg;          // the mixed channel tile: same layout, other descriptors
    const unsigned rs[2] = {(unsigned)p.t.range_stride[0], (unsigned)p.t.range_stride[1]};
    const unsigned chunk_stride = rs[0] + (p.t.NR > 1 ? rs[1] : 0);
    const int chs = (int)(r0 / chunk_stride);            // chunk over all sources
    r0 -= (unsigned)chs * chunk_stride;
    const int srcsel = chs / p.nch, ch = chs - srcsel * p.nch;
    const int range = (r0 >= rs[0]) ? 1 : 0;
    if (range) r0 -= rs[0];
    const int ntr = range ? p.t.NT2 : NT;
    const int per_m = 64 * 2 * ntr;
    const int per_pair = 8 * per_m;
    const int j = (int)(r0 / (unsigned)per_pair);
    int r1 = (int)(r0 - (unsigned)j * (unsigned)per_pair);
    const int m = r1 / per_m;
    r1 -= m * per_m;
    const int lane = r1 / (2 * ntr);
    r1 -= lane * 2 * ntr;
    const int t = r1 >> 1, gg = r1 & 1;
    const int k = lane >> 4, n = lane & 15;
    const int g = 2 * j + gg;
    if (g >= p.NG) return 0.f;
    const int kq = 4 * g + k;
    if (kq >= p.IBC * p.taps) return 0.f;                  // padding of the last k-group
    const int tf = range ? p.t.NT1 + t : t;                  // tile (accumulator slot) of the workgroup
    const int ds = mix ? 2 : tf;                           // descriptor slot: a mixed workgroup's slot NT1 is the mixed
    const int grp = n >> 3;                                // tile, its other slots are padding
    const int ob0 = (mix && tf != p.t.NT1) ? -1 : p.t.tile_ob[ds][grp];
    if (ob0 < 0) return 0.f;
    const int dblk = ob0 + (mix ? 0 : ytile * p.t.ob_step) + (n & 7);     // destination block channel
    const int kbl = kq / p.taps;
    const int tap = kq - kbl * p.taps;
    const int sblk = ch * p.IBC + kbl;                                  // source block channel
    const int hd = p.t.tile_half[ds][grp], hs = p.t.half_src[range];
    // which quaternion of the dual quaternion couples (source half hs) -> (destination half hd)
    int qsel = 0;                                                        // 0: Q, 1: Q2, -1: structural zero
    if (p.A == 8) {
        if (p.mode == 0) qsel = (hd == hs) ? 0 : (hd == 1 ? 1 : -1);     // y_p = Q x_p; y_d = Q2 x_p + Q x_d
        else qsel = (hd == hs) ? 0 : (hd == 0 ? 1 : -1);                 // dx_p = Q^ dy_p + Q2^ dy_d; dx_d = Q^ dy_d
    }
    if (qsel < 0) return 0.f;
    const int co = p.mode == 0 ? dblk : sblk;           // conv output / input block channel of the element
    const int ci = p.mode == 0 ? sblk : dblk;
    const int tp = p.mode == 0 ? tap : p.taps - 1 - tap;
    if (co >= p.OA || ci >= p.IA) return 0.f;
    const size_t e = ((size_t)co * p.IA + ci) * p.taps + tp;
    const WPtrs& w = p.w[p.mode == 0 ? set : srcsel];
    float a[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) a[c] = w.p[qsel * 4 + c][e];
    if (p.mode == 1) { a[1] = -a[1]; a[2] = -a[2]; a[3] = -a[3]; }      // conjugate
    return hcq_form_f(m, a);
}

__global__ __launch_bounds__(256) void hcq_pack_kernel(const HcqPackP p) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx < p.total) p.out[idx] = hcq_pack_value(p, idx);
}

// Every registered layer in ONE launch (once per optimiser step), balanced: blockIdx.x runs over the 256-float blocks of
// ALL entries back to back; starts[e] = first block of entry e (starts[nentries] = total).  (A (blocks, entries) grid sized
// for the largest entry launched mostly empty workgroups, a capped one looped: 60 us either way.)
__global__ __launch_bounds__(256) void hcq_pack_flat_kernel(const HcqPackP* __restrict__ table, const int* __restrict__ starts,
                                                            int nentries) {
    const int b = blockIdx.x;
    int lo = 0, hi = nentries;                       // last entry with starts[e] <= b
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (starts[mid] <= b) lo = mid; else hi = mid;
    }
    const HcqPackP& p = table[lo];
    const long long idx = (long long)(b - starts[lo]) * 256 + threadIdx.x;
    if (idx < p.total) p.out[idx] = hcq_pack_value(p, idx);
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
// The plan of (desc, mode, npair); modes and first_ok: hcq_conv.h.
HcqPlan hcq_plan(const seld_conv_desc* d, int mode, int npair, bool first_ok) {
    HcqPlan pl{};
    const bool pool = mode == 2;
    if (pool) mode = 0;
    const int A = d->algebra;
    if ((A != 4 && A != 8) || !hcq_same_geometry(d)) return pl;
    const int KH = d->k[0], KW = d->k[1];
    const int W = d->in[1], Himg = d->in[0];
    if (W % 64) return pl;
    const int Csrc = mode == 0 ? d->Cin : d->Cout, Cdst = mode == 0 ? d->Cout : d->Cin;
    const int IB = Csrc / A, OB = Cdst / A;
    const int taps = KH * KW;
    const int nsets = mode == 0 ? npair : 1, nsrc = mode == 1 ? npair : 1;
    const int dil = KW == 3 ? d->dil[1] : 0;
    const int dpad = KW == 3 ? (dil + 3) / 4 * 4 : 0;
    const int wext = 64 + 2 * dpad;
    // K chunk: candidates in order of preference; the input buffers of two workgroups per CU must fit (78 KB each)
    static const int cand11[] = {16, 24, 8, 0}, cand13[] = {8, 4, 0}, cand33[] = {4, 2, 1, 0};
    const int* cand = taps == 1 ? cand11 : (taps == 3 ? cand13 : cand33);
    int IBC = 0;
    size_t smem = 0;
    for (int i = 0; cand[i]; ++i) {
        if (IB % cand[i]) continue;
        const int nbuf = (IB / cand[i]) * nsrc > 1 ? 2 : 1;
        const size_t need = (size_t)nbuf * A * cand[i] * KH * wext * sizeof(float);
        if (need <= 78 * 1024) { IBC = cand[i]; smem = need; break; }
    }
    if (!IBC) return pl;
    // The 8-channel dual-quaternion first layer (ONE block channel: 9 of 12 k-slots used) stays on the persistent short-K
    // kernel hc_conv_smallk_kernel<12,3,3,4,18,9>: 610 us (530 inside the step) against 629 (571) for hcq_first_kernel
    // and 688 for hcq_conv_kernel at batch 32; 280 / 287 / 326 at 16.  With two block channels the fast product wins:
    // config 4's 16-channel layer (which does not fit that kernel's LDS) 1303 -> 405 us, config 2's quaternion layer
    // 342 -> 225.
    if (!pool && mode == 0 && taps == 9 && A == 8 && IB == 1 && Cdst == 192 && (long long)d->N * Himg * W >= 256 * 128 &&
        !env().conv_no_smallk) return pl;
    // channel tiles
    HcqP& k = pl.kp;
    HcqTiles& t = k.t;
    for (int i = 0; i < 3; ++i)
        for (int g = 0; g < 2; ++g) { t.tile_half[i][g] = 0; t.tile_ob[i][g] = -1; }
    if (A == 8) {
        t.NR = 2;
        // forward: range 0 = primal source (both destination halves), range 1 = dual source (dual destination only)
        // gradient: range 0 = dual source (both halves), range 1 = primal source (primal destination only)
        const int both = mode == 0 ? 1 : 0;           // destination half active in both ranges
        const int once = 1 - both;
        t.half_src[0] = mode == 0 ? 0 : 1;
        t.half_src[1] = 1 - t.half_src[0];
        if (OB % 16 != 0 && OB % 16 != 8) return pl;
        t.NT1 = 1; t.NT2 = 1; t.nreg = OB / 16; t.ob_step = 16;
        t.tile_half[0][0] = t.tile_half[0][1] = once; t.tile_ob[0][0] = 0; t.tile_ob[0][1] = 8;
        t.tile_half[1][0] = t.tile_half[1][1] = both; t.tile_ob[1][0] = 0; t.tile_ob[1][1] = 8;
        if (OB % 16 == 8) {                           // the last 8 block channels of both halves share one tile
            t.tile_half[2][0] = once; t.tile_ob[2][0] = OB - 8;
            t.tile_half[2][1] = both; t.tile_ob[2][1] = OB - 8;
            // 24 block channels: either ONE workgroup per position tile with three tiles (24 accumulators, the input
            // staged once: cnn.1 949 us against 1139), or the mixed tile in workgroups of its own (twice the
            // workgroups for layers with few position tiles: TCN data gradient 47.5 us against 68.6).  A forward PAIR
            // brings its own factor of two (two weight sets): skip || residual at batch 32 (256 position tiles) 39.8 ->
            // 32.3 us as 512 three-tile workgroups instead of 1024 two-tile ones, a third of them half padding
            const long long ptiles = (long long)d->N * Himg * W / 64;
            if (OB == 24 && ptiles * nsets >= 512) { t.NT2 = 2; t.ob_step = 0; }
            else t.mix = 1;
        }
        if (t.nreg == 0) return pl;
    } else {
        t.NR = 1; t.NT2 = 0;
        t.half_src[0] = t.half_src[1] = 0;
        if (OB % 32 == 0) { t.NT1 = 2; t.nreg = OB / 32; t.ob_step = 32; }
        else if (OB % 16 == 0) { t.NT1 = 1; t.nreg = OB / 16; t.ob_step = 16; }
        else return pl;
        for (int i = 0; i < t.NT1; ++i) { t.tile_ob[i][0] = 16 * i; t.tile_ob[i][1] = 16 * i + 8; }
    }
    const int NT = t.NT1 + t.NT2, mix = t.mix;
    // ---- the instantiation: tile program and table row ---------------------------------------------------------------
    pl.variant = t.NR == 2 ? (t.NT2 == 2 ? 0 : (mix ? 1 : 2)) : (t.NT1 == 2 ? 3 : 4);
    const int XI = (A * IBC * KH * (wext / 4) + 255) / 256;                   // staging items per thread
    pl.row = -1;
    for (int i = 0; i < HCQ_NINST && pl.row < 0; ++i) {
        const HcqInst& r = HCQ_INST[i];
        if (r.KH == KH && r.KW == KW && r.IBC == IBC && XI <= (t.NR == 2 ? r.XI8 : r.XI4)) pl.row = i;
    }
    if (pl.row < 0) return pl;
    pl.XI = t.NR == 2 ? HCQ_INST[pl.row].XI8 : HCQ_INST[pl.row].XI4;
    k.ytiles = t.nreg + mix; k.mix_ytile = mix ? t.nreg : -1;
    const long long ptot = (long long)d->N * Himg * W;
    const int NG = (IBC * taps + 3) / 4, NPAIR = (NG + 1) / 2;
    // first layers: one chunk, one channel tile, one weight set -> the row-walking kernels
    if (first_ok && mode == 0 && taps == 9 && IBC == IB && IB <= 2 && k.ytiles == 1 && nsets == 1 && !mix && Himg % HCQ_FIRST_R == 0 &&
        wext == 72) {
        pl.first_rows = HCQ_FIRST_R;
        pl.grid = dim3((unsigned)(ptot / 64 / HCQ_FIRST_R), 1, 1);
        const size_t rows = (size_t)A * IBC * (HCQ_FIRST_R + 2) * wext;
        pl.smem = pool ? (rows + (size_t)NT * 4 * 4 * 16 * 2 + (size_t)t.NR * NPAIR * 8 * 64 * 2) * sizeof(float)   // + statistics + one tile's fragments
                       : (rows + 4 * NT * 4 * 64 * 2) * sizeof(float);                                              // + statistics slots
    } else {
        if (pool) return pl;
        // LDS of hcq_conv_kernel = input buffers + fragment ring of two slots (a slot: the 8 forms of a pair of k-groups,
        // 4 KB per tile, or 4 forms).  The chunk stays the one chosen above (with two K ranges the chunk size decides the
        // order in which an accumulator meets them, i.e. the bits of the result).  The ring must not cost a resident workgroup
        // per CU (160 KB; registers allow 3 at most): whole pairs if they keep the count, else half pairs if they do (one
        // more barrier per pair).  Two exceptions, both measured (profiles/hcq_fragment_ring_shapes.md):
        //   * launches with mixed-tile workgroups (a third of their workgroups run one tile in range 0: 8 MFMAs per half-pair
        //     unit) are faster with whole pairs at two workgroups per CU than with half pairs at three: TCN 1x3 data
        //     gradient, halo 8, 39.8 us against 43.4 (41 to 42 before the ring);
        //   * quaternion 1-D layers keep per-wave global loads (GF): one range, one or two tiles and few chunks -- launches
        //     of about 10 us in which a barrier per pair costs what the L1 traffic saves (+0.2 ... -1.5 us with the ring).
        // A 1-D shape that no ring fits without losing a workgroup (1x3 forward, halo 12 to 16 or above 56) keeps global
        // loads as well; a 3x3 shape would take half pairs regardless (none does at the networks' widths).
        pl.gf = A == 4 && KH == 1;
        if (!pl.gf) {
            const auto wgs = [](size_t bytes) { const size_t n = (size_t)160 * 1024 / (bytes < 8192 ? 8192 : bytes); return n > 3 ? (size_t)3 : n; };
            const size_t wgs0 = wgs(smem);
            const size_t whole = (size_t)2 * 4096 * NT, halves = (size_t)2 * 2048 * NT;
            int half_slots = 0;
            if (wgs(smem + whole) >= wgs0 || (mix && wgs(smem + whole) >= 2)) half_slots = 0;
            else if (wgs(smem + halves) >= wgs0 || KH != 1) half_slots = 1;
            else pl.gf = true;
            if (!pl.gf) {
                k.ring_off = (int)smem;
                k.half_slots = half_slots;
                smem += half_slots ? halves : whole;
            }
        }
        if (smem < 8 * 1024) smem = 8 * 1024;                                 // statistics scratch of the epilogue
        pl.grid = dim3((unsigned)(ptot / 64), (unsigned)(k.ytiles * nsets), 1);
        pl.smem = smem;
    }
    pl.pool = pool;
    k.A = A; k.N = d->N; k.Csrc = Csrc; k.Cdst = Cdst; k.IB = IB; k.OB = OB;
    k.W = W; k.Himg = Himg; k.dil = dil; k.dpad = dpad; k.wext = wext; k.nch = IB / IBC;
    k.nsrc = nsrc;
    t.range_stride[0] = (long long)NPAIR * 8 * 64 * 2 * NT;
    t.range_stride[1] = (long long)NPAIR * 8 * 64 * 2 * t.NT2;
    t.ytile_stride = (long long)nsrc * k.nch * (t.range_stride[0] + (t.NR > 1 ? t.range_stride[1] : 0));
    t.set_stride = (long long)k.ytiles * t.ytile_stride;
    pl.pack_floats = (size_t)t.set_stride * nsets;
    HcqPackP& q = pl.pp;
    q.A = A; q.mode = mode; q.OA = d->Cout / A; q.IA = d->Cin / A; q.taps = taps;
    q.IBC = IBC; q.nch = k.nch; q.NG = NG; q.NPAIR = NPAIR; q.nsets = nsets; q.nsrc = nsrc;
    q.t = t;
    q.total = (long long)pl.pack_floats;
    pl.ok = 1;
    return pl;
}

// XI of (row, variant), 0: not instantiated
template <int I, int V> constexpr int hcq_xi() { return HCQ_TILEV[V].NR == 2 ? HCQ_INST[I].XI8 : HCQ_INST[I].XI4; }

template <int I, int V>
struct HcqLaunchConv {
    static int run(const HcqPlan& pl, hipStream_t st) {
        constexpr HcqInst R = HCQ_INST[I];
        constexpr HcqTileV T = HCQ_TILEV[V];
        constexpr int XI = hcq_xi<I, V>();
        if constexpr (XI > 0) {
            if constexpr (R.KH == 1) {                        // the global-load form exists for the shapes hcq_plan gives it to
                if (pl.gf) return hcq_launch_kernel(hcq_conv_kernel<R.KH, R.KW, R.IBC, T.NT1, T.NT2, T.NR, XI, T.MX, true>, pl, st, pl.kp);
            }
            return hcq_launch_kernel(hcq_conv_kernel<R.KH, R.KW, R.IBC, T.NT1, T.NT2, T.NR, XI, T.MX, false>, pl, st, pl.kp);
        }
        return SELD_EUNSUPPORTED;
    }
};

static int hcq_launch(const HcqPlan& pl, hipStream_t st) {
    if (pl.first_rows) return hcq_launch_first(pl, st);
    SELD_HCQ_DISPATCH(HcqLaunchConv, pl, st)
    return SELD_EUNSUPPORTED;
}

}  // namespace seld

using namespace seld;

static bool hcq_args_ok(const seld_conv_desc* d, int32_t mode, int32_t npair) {
    return hc_validate(d) == SELD_OK && mode >= 0 && mode <= 2 && npair >= 1 && npair <= 2;
}

extern "C" size_t seld_hcq_pack_floats(const seld_conv_desc* d, int32_t mode, int32_t npair) {
    if (!hcq_args_ok(d, mode, npair) || env().conv_no_hcq) return 0;
    const HcqPlan pl = hcq_plan(d, mode, npair);
    return pl.ok ? pl.pack_floats : 0;
}

extern "C" size_t seld_hcq_pack_entry_bytes(void) { return sizeof(HcqPackP); }

/* Kernel symbol (as rocprofv3 prints it) that seld_hcq_conv launches for (desc, mode, npair). */
extern "C" int seld_hcq_kernel_label(const seld_conv_desc* d, int32_t mode, int32_t npair, char* buf, int32_t buflen) {
    if (hc_validate(d) != SELD_OK || !buf || buflen < 64) return SELD_EINVAL;
    const HcqPlan pl = hcq_plan(d, mode, npair);
    if (!pl.ok) return SELD_EUNSUPPORTED;
    const HcqInst& r = HCQ_INST[pl.row];
    const HcqTileV& v = HCQ_TILEV[pl.variant];
    if (pl.first_rows)   // (hcq_first_pool_kernel: the WY / FIN arguments depend on the entry point's pointers)
        snprintf(buf, buflen, pl.pool ? "hcq_first_pool_kernel<%d, %d, %d, %d, %d>" : "hcq_first_kernel<%d, %d, %d, %d, %d>", r.IBC,
                 v.NT1, v.NT2, v.NR, pl.first_rows);
    else
        snprintf(buf, buflen, "hcq_conv_kernel<%d, %d, %d, %d, %d, %d, %d, %s, %s>", r.KH, r.KW, r.IBC, v.NT1, v.NT2, v.NR, pl.XI,
                 v.MX ? "true" : "false", pl.gf ? "true" : "false");
    return SELD_OK;
}

/* Host-only: the launch seld_hcq_conv (mode 0 / 1) or seld_hcq_first_pool (mode 2) makes for (desc, mode, npair). */
extern "C" int seld_hcq_launch_shape(const seld_conv_desc* d, int32_t mode, int32_t npair, int32_t out[6]) {
    if (!hcq_args_ok(d, mode, npair) || !out) return SELD_EINVAL;
    const HcqPlan pl = hcq_plan(d, mode, npair);
    if (!pl.ok) return SELD_EUNSUPPORTED;
    out[0] = (int32_t)pl.grid.x; out[1] = (int32_t)pl.grid.y; out[2] = (int32_t)pl.smem;
    out[3] = pl.kp.ring_off; out[4] = pl.kp.half_slots; out[5] = pl.first_rows;
    return SELD_OK;
}

/* Fill one table entry (host memory, seld_hcq_pack_entry_bytes() bytes) for seld_hcq_pack_flat. */
extern "C" int seld_hcq_pack_entry(const seld_conv_desc* d, int32_t mode, int32_t npair, const float* const wA[8],
                                   const float* const wB[8], float* wpack, void* entry) {
    if (!hcq_args_ok(d, mode, npair) || !wA || !wpack || !entry || (npair == 2 && !wB)) return SELD_EINVAL;
    HcqPlan pl = hcq_plan(d, mode, npair);
    if (!pl.ok) return SELD_EUNSUPPORTED;
    for (int i = 0; i < 8; ++i) {
        pl.pp.w[0].p[i] = i < d->algebra ? wA[i] : nullptr;
        pl.pp.w[1].p[i] = (npair == 2 && i < d->algebra) ? wB[i] : nullptr;
    }
    pl.pp.out = wpack;
    memcpy(entry, &pl.pp, sizeof(HcqPackP));
    return SELD_OK;
}

extern "C" int seld_hcq_pack(const seld_conv_desc* d, int32_t mode, int32_t npair, const float* const wA[8],
                             const float* const wB[8], float* wpack, void* stream) {
    HcqPackP e;
    const int rc = seld_hcq_pack_entry(d, mode, npair, wA, wB, wpack, &e);
    if (rc != SELD_OK) return rc;
    const unsigned blocks = (unsigned)((e.total + 255) / 256);
    hipLaunchKernelGGL(hcq_pack_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, e);
    return check_launch();
}

/* Every entry of a DEVICE table in one launch: starts_dev[e] = first 256-float block of entry e, starts_dev[nentries] =
 * total_blocks. */
extern "C" int seld_hcq_pack_flat(const void* table_dev, const int32_t* starts_dev, int32_t nentries, int32_t total_blocks,
                                  void* stream) {
    if (!table_dev || !starts_dev || nentries <= 0 || total_blocks <= 0) return SELD_EINVAL;
    hipLaunchKernelGGL(hcq_pack_flat_kernel, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const HcqPackP*)table_dev, starts_dev, nentries);
    return check_launch();
}

extern "C" int seld_hcq_conv(const seld_conv_desc* d, int32_t mode, int32_t npair, const float* x, const float* x2,
                             const float* wpack, float* const y[2], const float* const bias[2],
                             const int32_t epilogue[2], const float* const addend[2], float* const stats[2],
                             void* stream) {
    if (hc_validate(d) != SELD_OK || !x || !wpack || !y || !y[0]) return SELD_EINVAL;
    if ((mode != 0 && mode != 1) || npair < 1 || npair > 2) return SELD_EINVAL;
    if (mode == 1 && npair == 2 && !x2) return SELD_EINVAL;
    // (same packed weights for both kernels of a first-layer shape)
    HcqPlan pl = hcq_plan(d, mode, npair, !(epilogue && (epilogue[0] & ~SELD_EPI_STATS)));
    if (!pl.ok) return SELD_EUNSUPPORTED;
    const int nsets = mode == 0 ? npair : 1;
    for (int s = 0; s < 2; ++s) {
        const bool on = s < nsets;
        pl.kp.dst[s] = on ? y[s] : nullptr;
        pl.kp.bias[s] = (on && bias) ? bias[s] : nullptr;
        pl.kp.epilogue[s] = (on && epilogue) ? epilogue[s] : 0;
        pl.kp.addend[s] = (on && addend) ? addend[s] : nullptr;
        pl.kp.stats[s] = (on && stats) ? stats[s] : nullptr;
        if (on && !pl.kp.dst[s]) return SELD_EINVAL;
        if ((pl.kp.epilogue[s] & SELD_EPI_ADD) && !pl.kp.addend[s]) return SELD_EINVAL;
        if ((pl.kp.epilogue[s] & SELD_EPI_STATS) && !pl.kp.stats[s]) return SELD_EINVAL;
    }
    pl.kp.src = x;
    pl.kp.src2 = x2;
    pl.kp.wpack = wpack;
    return hcq_launch(pl, (hipStream_t)stream);
}
