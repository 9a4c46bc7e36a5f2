// Log-power and first-order-Ambisonics intensity-vector features of complex spectra, linear in frequency or projected
// onto bands (a mel filterbank): the standard SELD input, computed from the planes seld_stft_complex_ws writes.
//
// z (2C, bins, frames): plane c = Re Z of channel c, plane C + c = Im Z.  Per bin k of a group of four channels
// [W, D1, D2, D3]:  p_c = |Z_c|^2,  E = eps + |W|^2 + (|D1|^2 + |D2|^2 + |D3|^2) / 3,  i_d = Re(conj(W) D_d) / E.
// Linear form: out = log(p + eps) / i_d per (bin, frame).  Banded form: P[m] = sum_k fb[m,k] p[k], I_d[m] = sum_k fb[m,k]
// i_d[k] -- normalised per bin, then projected --, out = log(P + eps) / I_d.
//
// HBM-bound VALU work.  Frames are the contiguous axis of z and out, so lanes run along frames and every load and store
// is one coalesced row segment (rows are dword-aligned only: bins * frames is arbitrary, nothing wider is assumed).
// Banded form: one wave owns kBandsPerWave bands of one 64-frame stretch of one unit (a group of four channels, or one
// channel for log-power alone); per bin of the band it loads the unit's planes, the weight fb[m,k] is wave-uniform, the
// band sums (4 powers, 3 intensity components) stay in registers and are accumulated in the band's bin order, so the
// result does not depend on the launch geometry.  A workgroup's waves take interleaved neighbouring bands: the bins two
// neighbouring triangles share are re-read while they are still in L2.  No LDS, no atomics, no cross-lane operation:
// results are run-to-run identical.  Lanes beyond the last frame read the last frame and store nothing.
// Every multiply-add is written out (fmaf) and contraction is off, so one quantity is the same bits in every kind, layout
// and instantiation, and negating a channel negates exactly what depends on its sign.
#include "common.h"

namespace seld {
namespace {

constexpr int kWaves = 4;             // waves of a workgroup of the banded kernel
constexpr int kBandsPerWave = 2;      // bands m, m + kWaves of the workgroup's kWaves * kBandsPerWave consecutive bands

// Powers p[j] of the NCH channels of one unit at element e of their planes and, for a group, the normalised intensity.
template <int NCH>
__device__ __forceinline__ void bin_values(const float* __restrict__ re, const float* __restrict__ im, size_t plane,
                                           size_t e, float eps, float (&p)[NCH], float (&iv)[3]) {
#pragma clang fp contract(off)
    float zr[NCH], zi[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        zr[j] = re[j * plane + e];
        zi[j] = im[j * plane + e];
        p[j] = fmaf(zr[j], zr[j], zi[j] * zi[j]);
    }
    if constexpr (NCH == 4) {
        const float inv = 1.0f / (eps + p[0] + (p[1] + p[2] + p[3]) / 3.0f);
#pragma unroll
        for (int d = 0; d < 3; ++d) iv[d] = fmaf(zr[0], zr[d + 1], zi[0] * zi[d + 1]) * inv;
    }
}

// The planes of unit u at element e of an out plane of `oplane` floats.  Log-power of channel c is plane c wherever it
// is kept (every channel, or layout 1: the group's W); the intensity planes follow the layouts of seld_hip.h.
template <int NCH>
__device__ __forceinline__ void store_unit(float* __restrict__ out, int C, size_t oplane, size_t e, int u, int kind,
                                           int layout, float eps, const float (&P)[NCH], const float (&I)[3]) {
#pragma clang fp contract(off)
    if constexpr (NCH == 1) {
        out[(size_t)u * oplane + e] = logf(P[0] + eps);
    } else {
        const int nlp = kind == SELD_FEAT_IV ? 0 : layout == SELD_FEAT_LAYOUT_QUATERNION ? 1 : 4;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nlp) out[(size_t)(4 * u + j) * oplane + e] = logf(P[j] + eps);
        const int iv0 = kind == SELD_FEAT_IV ? 3 * u : layout == SELD_FEAT_LAYOUT_QUATERNION ? 4 * u + 1 : C + 3 * u;
#pragma unroll
        for (int d = 0; d < 3; ++d) out[(size_t)(iv0 + d) * oplane + e] = I[d];
    }
}

// fb == NULL: one (bin, frame) element of one unit per lane.  grid (ceil(plane / 256), units).
template <int NCH>
__global__ __launch_bounds__(256) void features_linear_kernel(const float* __restrict__ z, int C, size_t plane, int kind,
                                                              int layout, float eps, float* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= plane) return;
    const int u = blockIdx.y;
    const float* re = z + (size_t)u * NCH * plane;
    float p[NCH], iv[3] = {0.f, 0.f, 0.f};
    bin_values<NCH>(re, re + (size_t)C * plane, plane, e, eps, p, iv);
    store_unit<NCH>(out, C, plane, e, u, kind, layout, eps, p, iv);
}

// grid (ceil(frames / 64), ceil(bands / (kWaves * kBandsPerWave)), units), kWaves * 64 threads.
template <int NCH>
__global__ __launch_bounds__(kWaves * 64) void features_banded_kernel(const float* __restrict__ z, int C, int bins,
                                                                      int frames, int kind, int layout,
                                                                      const float* __restrict__ fb,
                                                                      const int32_t* __restrict__ band_lo,
                                                                      const int32_t* __restrict__ band_hi, int bands,
                                                                      float eps, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int f = blockIdx.x * 64 + lane;
    const bool live = f < frames;
    const int fc = live ? f : frames - 1;
    const int u = blockIdx.z;
    const size_t plane = (size_t)bins * frames;
    const float* re = z + (size_t)u * NCH * plane + fc;
    const float* im = re + (size_t)C * plane;
    for (int i = 0; i < kBandsPerWave; ++i) {
        const int m = blockIdx.y * (kWaves * kBandsPerWave) + i * kWaves + wave;
        if (m >= bands) break;                               // wave-uniform
        const int lo = band_lo[m] > 0 ? band_lo[m] : 0;
        const int hi = band_hi[m] < bins ? band_hi[m] : bins;
        const float* w = fb + (size_t)m * bins;
        float P[NCH], I[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NCH; ++j) P[j] = 0.f;
#pragma unroll 2
        for (int k = lo; k < hi; ++k) {
            float p[NCH], iv[3] = {0.f, 0.f, 0.f};
            bin_values<NCH>(re, im, plane, (size_t)k * frames, eps, p, iv);
            const float wk = w[k];
#pragma unroll
            for (int j = 0; j < NCH; ++j) P[j] = fmaf(wk, p[j], P[j]);
#pragma unroll
            for (int d = 0; d < 3; ++d) I[d] = fmaf(wk, iv[d], I[d]);
        }
        if (live) store_unit<NCH>(out, C, (size_t)bands * frames, (size_t)m * frames + f, u, kind, layout, eps, P, I);
    }
}

int feature_channels(long long C, int kind, int layout) {
    if (C < 1 || kind < SELD_FEAT_LOGPOWER || kind > SELD_FEAT_LOGPOWER_IV ||
        (layout != SELD_FEAT_LAYOUT_GROUPED && layout != SELD_FEAT_LAYOUT_QUATERNION))
        return SELD_EINVAL;
    if (kind != SELD_FEAT_LOGPOWER && C % 4 != 0) return SELD_EINVAL;
    if (layout == SELD_FEAT_LAYOUT_QUATERNION && kind != SELD_FEAT_LOGPOWER_IV) return SELD_EINVAL;
    const long long n = kind == SELD_FEAT_LOGPOWER ? C
                        : kind == SELD_FEAT_IV     ? 3 * (C / 4)
                        : layout == SELD_FEAT_LAYOUT_QUATERNION ? C : C + 3 * (C / 4);
    return n > 0x7fffffffLL ? SELD_EUNSUPPORTED : (int)n;
}

}  // namespace
}  // namespace seld
using namespace seld;

extern "C" int seld_spatial_features_channels(int32_t C, int32_t kind, int32_t layout) {
    return feature_channels(C, kind, layout);
}

extern "C" int seld_spatial_features(const float* z, int32_t C, int32_t bins, int32_t frames, int32_t kind, int32_t layout,
                                     const float* fb, const int32_t* band_lo, const int32_t* band_hi, int32_t bands,
                                     float eps, float* out, void* stream) {
    if (!z || !out || bins < 1 || frames < 1 || bands < 1 || !(eps > 0.f)) return SELD_EINVAL;
    const int planes = feature_channels(C, kind, layout);
    if (planes < 0) return planes;
    if (fb ? (!band_lo || !band_hi) : bands != bins) return SELD_EINVAL;
    const bool group = kind != SELD_FEAT_LOGPOWER;
    const int units = group ? C / 4 : C;
    const size_t plane = (size_t)bins * (size_t)frames;
    if (units > 65535 || plane >= ((size_t)1 << 31) || (size_t)bands * (size_t)frames >= ((size_t)1 << 31))
        return SELD_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    if (!fb) {
        const dim3 grid((unsigned)((plane + 255) / 256), units);
        if (group)
            hipLaunchKernelGGL(features_linear_kernel<4>, grid, dim3(256), 0, s, z, C, plane, kind, layout, eps, out);
        else
            hipLaunchKernelGGL(features_linear_kernel<1>, grid, dim3(256), 0, s, z, C, plane, kind, layout, eps, out);
        return check_launch();
    }
    const int per_block = kWaves * kBandsPerWave;
    const dim3 grid((frames + 63) / 64, (bands + per_block - 1) / per_block, units);
    if (grid.y > 65535) return SELD_EUNSUPPORTED;
    if (group)
        hipLaunchKernelGGL(features_banded_kernel<4>, grid, dim3(kWaves * 64), 0, s, z, C, bins, frames, kind, layout, fb,
                           band_lo, band_hi, bands, eps, out);
    else
        hipLaunchKernelGGL(features_banded_kernel<1>, grid, dim3(kWaves * 64), 0, s, z, C, bins, frames, kind, layout, fb,
                           band_lo, band_hi, bands, eps, out);
    return check_launch();
}
