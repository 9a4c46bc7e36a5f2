// What the forward / data-gradient block-matrix kernels share: hc_conv_kernel (hc_conv_fwd.hip) and hc_conv_vec_kernel
// (hc_conv_vec.hip) the tile origin, the K range, its dispatch, the accumulator clear and the epilogue; these two and
// hc_conv_smallk_kernel (hc_conv_smallk.hip) the statistics fold.  Staging, trackers and pipeline loops are each kernel's own.
#pragma once
#include <type_traits>
#include "hc_common.h"

namespace seld {

// ---- tile origin ----------------------------------------------------------------------------------------------------------
// A workgroup owns channels [c0, c0 + BC) and positions [p0, p0 + BP).  Position -> (image relative to img0, offset in
// image) without per-lane 64-bit division: the tile starts at (img0, rem0) (scalar), a lane adds its local index and wraps
// (32-bit divide only when an image is shorter than the tile).  The buffer descriptor's base stays with the kernel
// (hc_conv_vec_kernel bases it one image earlier).
template <int BP>
struct ConvOrigin {
    int c0;
    long long p0, img0;
    int rem0, dstS;
    __device__ __forceinline__ void decode(int local, int* dimg, int* rem) const {
        int r = rem0 + local;
        int di = 0;
        if (dstS >= BP) {
            if (r >= dstS) { r -= dstS; di = 1; }
        } else {
            di = r / dstS;
            r -= di * dstS;
        }
        *dimg = di;
        *rem = r;
    }
};
template <int BC, int BP>
__device__ __forceinline__ ConvOrigin<BP> conv_origin(const ConvP& p) {
    ConvOrigin<BP> o;
    o.c0 = blockIdx.y * BC;
    o.p0 = (long long)blockIdx.x * BP;
    o.dstS = p.dstS;
    o.img0 = o.p0 / o.dstS;
    o.rem0 = (int)(o.p0 - o.img0 * o.dstS);
    return o;
}

// ---- K range of a workgroup (dual-quaternion zero quadrant) ---------------------------------------------------------------
// Dual quaternion: the first half of the channels (primal part) sees a structurally-zero K half (skip_mode 1, forward; the
// data gradient, skip_mode 2, mirrors it: the dual channels see zeros in the lower K half).  Tiles are contiguous channel
// ranges.  UNIT: what a K chunk must align to (16; hc_conv_vec_kernel: its chunk).
// mixed_wg: the workgroup's lower tiles are primal and its upper tiles dual, so half of its tiles skip the zero quadrant's
// chunks, which start (forward) or end (data gradient) at chunk csplit (any other straddle just multiplies by the staged
// zeros).
struct ConvKRange {
    int kbeg, kend;
    bool mixed_wg;
    int csplit;                // first chunk of the upper K half
};
template <int BC, int CT, int UNIT>
__device__ __forceinline__ ConvKRange conv_k_range(const ConvP& p, int c0) {
    const int half_c = p.Cdst >> 1;
    const int half_k = p.Ktot >> 1;
    const bool halves_aligned = (p.skip_mode != 0) && (half_k % UNIT == 0) && (half_c % 16 == 0);
    ConvKRange k;
    k.kbeg = 0;
    k.kend = p.Ktot;
    if (halves_aligned) {
        if (p.skip_mode == 1 && c0 + BC <= half_c) k.kend = half_k;      // all channels primal
        if (p.skip_mode == 2 && c0 >= half_c) k.kbeg = half_k;           // all channels dual
    }
    k.mixed_wg = halves_aligned && (CT % 2 == 0) && (c0 + BC / 2 == half_c);
    k.csplit = UNIT == 16 ? (half_k - k.kbeg) >> 4 : (half_k - k.kbeg) / UNIT;
    return k;
}

// The K loop is run as up to two consecutive loops, each with a compile-time set of channel tiles [J0, J1): a mixed
// workgroup computes all of its tiles over one K half and only half of them over the other.  Each loop body is
// straight-line code (no per-tile branches, accumulators stay in place).  run(cbeg, cend, J0c, J1c) is the kernel's loop
// over chunks [cbeg, cend).
// REPS = 2, a pair (hc_conv_vec_kernel): the range is walked twice.  A data-gradient pair goes on into the same accumulators
// -- one loop of twice the length, or the two loops again; a forward pair calls between() after the first walk (slot 0's
// epilogue and the accumulator clear).  Straight-line repeats, never a loop over the repeats: that cost the 12-tile
// kernels 100+ VGPRs.
template <int CT, int MODE, int REPS, class Run, class Between>
__device__ __forceinline__ void conv_run_k_range(const ConvKRange& k, int skip_mode, int nchunks, Run&& run, Between&& between) {
    using IC0 = std::integral_constant<int, 0>;
    using ICH = std::integral_constant<int, CT / 2>;
    using ICT = std::integral_constant<int, CT>;
    static_assert(REPS == 1 || REPS == 2, "one convolution or a pair");
    constexpr bool FWD2 = REPS == 2 && MODE == MODE_FWD, DGRAD2 = REPS == 2 && MODE == MODE_DGRAD;
    if (k.mixed_wg) {
        if (skip_mode == 1) {                                 // forward: primal tiles (lower half) see zeros there
            run(0, k.csplit, IC0{}, ICT{});
            run(k.csplit, nchunks, ICH{}, ICT{});
            if (FWD2) {
                between();
                run(0, k.csplit, IC0{}, ICT{});
                run(k.csplit, nchunks, ICH{}, ICT{});
            }
        } else {                                              // dgrad: dual tiles (upper half) see zeros in the lower K half
            run(0, k.csplit, IC0{}, ICH{});
            run(k.csplit, nchunks, IC0{}, ICT{});
            if (DGRAD2) {
                run(0, k.csplit, IC0{}, ICH{});
                run(k.csplit, nchunks, IC0{}, ICT{});
            }
        }
    } else if (FWD2) {
        run(0, nchunks, IC0{}, ICT{});
        between();
        run(0, nchunks, IC0{}, ICT{});
    } else {
        run(0, (DGRAD2 ? 2 : 1) * nchunks, IC0{}, ICT{});
    }
}
template <int CT, int MODE, class Run>
__device__ __forceinline__ void conv_run_k_range(const ConvKRange& k, int skip_mode, int nchunks, Run&& run) {
    conv_run_k_range<CT, MODE, 1>(k, skip_mode, nchunks, run, [] {});
}

template <int PT, int CT>
__device__ __forceinline__ void conv_zero_acc(floatx4 (&acc)[PT][CT]) {
#pragma unroll
    for (int i = 0; i < PT; ++i)
#pragma unroll
        for (int j = 0; j < CT; ++j) acc[i][j] = (floatx4){0.f, 0.f, 0.f, 0.f};
}

// ---- BatchNorm statistics: partial sums of a workgroup -> one replica row -------------------------------------------------
// Lanes fr, fr + 16, fr + 32, fr + 48 hold the same channel and the waves hold different positions: fold the four lanes and
// let lane fk == 0 put the wave's sums of the tile's channel row `row` into red[wave][BC][2].  s1 and s2 are references on
// purpose: taken by value, the copies changed how the compiler pairs and contracts the callers' s1 / s2 chains (the
// o.x * o.x + ... sums got other fused multiply-adds than before, and the statistics other bits).
template <int BC>
__device__ __forceinline__ void conv_stats_put(float* red, int wave, int row, int fk, float& s1, float& s2) {
    s1 += __shfl_xor(s1, 16, 64);
    s1 += __shfl_xor(s1, 32, 64);
    s2 += __shfl_xor(s2, 16, 64);
    s2 += __shfl_xor(s2, 32, 64);
    if (fk == 0) {
        red[(wave * BC + row) * 2 + 0] = s1;
        red[(wave * BC + row) * 2 + 1] = s2;
    }
}
// Then: the four waves' sums in ascending wave order, and one atomic pair per channel per workgroup, spread over
// SELD_STATS_REPLICAS rows so that the thousands of workgroups of a layer do not serialise on 2*C addresses.
template <int BC>
__device__ __forceinline__ void conv_stats_flush(const float* red, float* stats, int Cdst, int c0, int tid) {
    __syncthreads();
    float* rep = stats + (size_t)(blockIdx.x % SELD_STATS_REPLICAS) * 2 * Cdst;
    for (int t = tid; t < BC; t += 256) {
        const int ch = c0 + t;
        if (ch < Cdst) {
            float a1 = 0.f, a2 = 0.f;
#pragma unroll
            for (int wv = 0; wv < 4; ++wv) {
                a1 += red[(wv * BC + t) * 2 + 0];
                a2 += red[(wv * BC + t) * 2 + 1];
            }
            atomicAdd(rep + ch, a1);
            atomicAdd(rep + Cdst + ch, a2);
        }
    }
}

// ---- epilogue -------------------------------------------------------------------------------------------------------------
// Where a result goes: slot 0, or the second convolution of a forward pair.
struct ConvOut {
    float* dst;
    const float* addend;
    const float* bias;
    float* stats;
    int epilogue;
};
__device__ __forceinline__ ConvOut conv_out(const ConvP& p, int slot) {
    return slot ? ConvOut{p.dst2, p.addend2, p.bias2, p.stats2, p.epilogue2} : ConvOut{p.dst, p.addend, p.bias, p.stats, p.epilogue};
}

// Lane (fr, fk) of wave `wave` holds positions prow .. prow + 3 (the four registers) of channel c0 + j*16 + fr in acc[i][j]:
// o = v + bias, then + addend, then + the old value; one 16-byte store.  SCALAR: dstS need not be a multiple of 4, the four
// positions are then stored one by one (each with its own image / offset).  red: LDS scratch [4][BC][2] of the statistics.
template <int CT, int PT, bool SCALAR>
__device__ __forceinline__ void conv_epilogue(const ConvP& p, const ConvOrigin<PT * 64>& og, const ConvOut& out,
                                              const floatx4 (&acc)[PT][CT], float* red, int tid) {
    constexpr int BC = CT * 16;
    // read once: the atomics below keep the compiler from carrying a load through `p` across them
    const int Cdst = p.Cdst, dstS = p.dstS, epi = out.epilogue, c0 = og.c0;
    const long long Ptot = p.Ptot, p0 = og.p0, img0 = og.img0;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 15, fk = lane >> 4;
    const bool vec_ok = SCALAR ? (dstS % 4 == 0) : true;
    // element offset of (first image of the tile, channel 0, position 0) and, per position tile i, of this
    // lane's 4 positions relative to it
    float* const dst0 = out.dst + (size_t)img0 * Cdst * dstS;
    const float* const add0 = out.addend ? out.addend + (size_t)img0 * Cdst * dstS : nullptr;
    int poff[PT];
#pragma unroll
    for (int i = 0; i < PT; ++i) {
        int dimg, rem;
        og.decode(wave * (PT * 16) + i * 16 + fk * 4, &dimg, &rem);
        poff[i] = dimg * Cdst * dstS + rem;
    }
#pragma unroll
    for (int j = 0; j < CT; ++j) {
        const int ch = c0 + j * 16 + fr;
        const bool chok = ch < Cdst;
        const float bvv = (chok && out.bias) ? out.bias[ch] : 0.0f;
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < PT; ++i) {
            const long long pos = p0 + wave * (PT * 16) + i * 16 + fk * 4;
            floatx4 v = acc[i][j];
            if (chok && pos < Ptot) {
                if (vec_ok) {
                    const size_t off = (size_t)(poff[i] + ch * dstS);
                    float4 o = make_float4(v[0] + bvv, v[1] + bvv, v[2] + bvv, v[3] + bvv);
                    if (epi & SELD_EPI_ADD) {
                        float4 ad = *reinterpret_cast<const float4*>(add0 + off);
                        o.x += ad.x; o.y += ad.y; o.z += ad.z; o.w += ad.w;
                    }
                    if (epi & SELD_EPI_ACCUMULATE) {
                        float4 old = *reinterpret_cast<const float4*>(dst0 + off);
                        o.x += old.x; o.y += old.y; o.z += old.z; o.w += old.w;
                    }
                    *reinterpret_cast<float4*>(dst0 + off) = o;
                    s1 += o.x + o.y + o.z + o.w;
                    s2 += o.x * o.x + o.y * o.y + o.z * o.z + o.w * o.w;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        long long pr = pos + r;
                        if (pr < Ptot) {
                            long long img = pr / dstS;
                            int rem = (int)(pr - img * dstS);
                            size_t off = ((size_t)img * Cdst + ch) * dstS + rem;
                            float o = v[r] + bvv;
                            if (epi & SELD_EPI_ADD) o += out.addend[off];
                            if (epi & SELD_EPI_ACCUMULATE) o += out.dst[off];
                            out.dst[off] = o;
                            s1 += o;
                            s2 += o * o;
                        }
                    }
                }
            }
        }
        if (epi & SELD_EPI_STATS) conv_stats_put<BC>(red, wave, j * 16 + fr, fk, s1, s2);
    }
    if (epi & SELD_EPI_STATS) conv_stats_flush<BC>(red, out.stats, Cdst, c0, tid);
}

}  // namespace seld
