// Hypercomplex (real / quaternion) TRANSPOSED convolution, gfx950 (quaternion_ops.py:149-171 of the reference).
//
//     y[n][co][oh][ow] = bias[co] + sum_{ci, kh, kw} u[n][ci][ih][iw] * M[ci][co][kh][kw],
//     oh = ih*sh - ph + kh*dh,   ow = iw*sw - pw + kw*dw
//
// M (Cin, Cout, kh, kw) is the Hamilton block matrix of the component tensors (Cin/A, Cout/A, kh, kw), the same
// arrangement as the forward convolution's.
//
// Forward: hc_tconv_kernel, the stride-phase implicit GEMM of hc_phase_gemm.h on two axes (phase map, weights read
// transposed); the kernel body, the per-axis phase tables, the tile choice and the launch are described and live there.
// This file keeps the descriptor checks of the 2-D entry points and the backward routing: the input gradient is the
// forward convolution of the mirrored descriptor (hc_conv_fwd_out), the weight gradient its weight gradient
// (hc_wgrad_out), the bias gradient tconv_bias_grad_kernel.
//
// The forward uses no float atomics: run-to-run bit-identical.
#include "hc_phase_gemm.h"

namespace seld {

template <int CT, int PT>
__global__ __launch_bounds__(256) void hc_tconv_kernel(const PgP<2> p) { pg_gemm<CT, PT, true, 2>(p); }

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
// Output extent per axis: (in - 1)*s - 2p + d*(k - 1) + op + 1; PyTorch's rule: op < s or op < d.
static int tconv_validate(const seld_conv_desc* d, const int32_t op[2], int out[2]) {
    int rc = hc_validate(d);
    if (rc) return rc;
    if (!op) return SELD_EINVAL;
    for (int i = 0; i < 2; ++i) {
        if (op[i] < 0 || (op[i] >= d->stride[i] && op[i] >= d->dil[i])) return SELD_EINVAL;
        out[i] = (d->in[i] - 1) * d->stride[i] - 2 * d->pad[i] + d->dil[i] * (d->k[i] - 1) + op[i] + 1;
        if (out[i] <= 0) return SELD_EINVAL;
    }
    if (d->ndim == 1 && (d->in[0] != 1 || d->k[0] != 1 || d->stride[0] != 1 || d->pad[0] != 0 || op[0] != 0))
        return SELD_EINVAL;
    return SELD_OK;
}

// the phase map (Cin, in) -> (Cout, out) of the shared plan, on two axes
static void tconv_fill(PgP<2>& p, const seld_conv_desc* d, const int out[2], const float* const w[8]) {
    PgGeom<2> g;
    g.A = d->algebra; g.N = d->N; g.Ci = d->Cin; g.Co = d->Cout;
    for (int i = 0; i < 2; ++i) {
        g.in[i] = d->in[i]; g.out[i] = out[i];
        g.k[i] = d->k[i]; g.s[i] = d->stride[i]; g.p[i] = d->pad[i]; g.d[i] = d->dil[i];
    }
    pg_fill(p, g, true, w);
}

// Limits of the phase kernel's addressing: per-axis stride <= PG_MAXS (phase tables), one output image addressed with
// 32-bit offsets like the input, and the input images one tile spans addressed with 32-bit byte offsets.
static int tconv_addressable(const seld_conv_desc* d, const int out[2]) {
    if (d->algebra == 8) return SELD_EUNSUPPORTED;            // no dual-quaternion transposed convolution in the reference
    if (d->stride[0] > PG_MAXS || d->stride[1] > PG_MAXS) return SELD_EUNSUPPORTED;
    if ((long long)d->Cout * out[0] * out[1] >= (1LL << 28)) return SELD_EUNSUPPORTED;
    PgP<2> p{};
    tconv_fill(p, d, out, nullptr);
    return pg_addressable(p);
}

// the four tiles of the 2-D tile choice
static int tconv_launch(const PgP<2>& p, hipStream_t st) {
    const PgCfg c = pg_cfg(p, false);
    if (c.ct == 12) return pg_launch(hc_tconv_kernel<12, 1>, c, p, st);
    if (c.ct == 2) return pg_launch(hc_tconv_kernel<2, 4>, c, p, st);
    if (c.ct == 1) return pg_launch(hc_tconv_kernel<1, 4>, c, p, st);
    return pg_launch(hc_tconv_kernel<4, 4>, c, p, st);
}

// Reduction over batch and positions of dy (N, C, S) per channel, added to out[c]: one workgroup per channel, fixed order.
__global__ __launch_bounds__(256) void tconv_bias_grad_kernel(const float* __restrict__ dy, int N, int C, long long S,
                                                              float* __restrict__ out) {
    const int c = blockIdx.x;
    float s = 0.f;
    for (int n = 0; n < N; ++n) {
        const float* row = dy + ((size_t)n * C + c) * S;
        for (long long i = threadIdx.x; i < S; i += 256) s += row[i];
    }
    __shared__ float red[4];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[c] += red[0] + red[1] + red[2] + red[3];
}

// the mirrored convolution: input = the transposed convolution's output, output = its input, same component tensors
static seld_conv_desc tconv_mirror(const seld_conv_desc* d, const int out[2]) {
    seld_conv_desc m = *d;
    m.Cin = d->Cout; m.Cout = d->Cin;
    m.in[0] = out[0]; m.in[1] = out[1];
    return m;
}

}  // namespace seld

using namespace seld;

extern "C" int seld_hc_conv_transpose_out_shape(const seld_conv_desc* d, const int32_t out_pad[2], int32_t out[2]) {
    int o[2];
    const int rc = tconv_validate(d, out_pad, o);
    if (rc) return rc;
    if (out) { out[0] = o[0]; out[1] = o[1]; }
    return SELD_OK;
}

extern "C" int seld_hc_conv_transpose_fwd(const seld_conv_desc* d, const int32_t out_pad[2], const float* x,
                                          const float* const w[8], const float* bias, float* y, void* stream) {
    int o[2];
    int rc = tconv_validate(d, out_pad, o);
    if (rc) return rc;
    if (!x || !w || !y) return SELD_EINVAL;
    rc = tconv_addressable(d, o);
    if (rc) return rc;
    PgP<2> p{};
    tconv_fill(p, d, o, w);
    p.x = x; p.bias = bias; p.y = y;
    return tconv_launch(p, (hipStream_t)stream);
}

// dx = conv(dy, M) with the same stride / padding / dilation, cut to the transposed convolution's input extent
extern "C" int seld_hc_conv_transpose_bwd_data(const seld_conv_desc* d, const int32_t out_pad[2], const float* dy,
                                               const float* const w[8], float* dx, void* stream) {
    int o[2];
    int rc = tconv_validate(d, out_pad, o);
    if (rc) return rc;
    if (!dy || !w || !dx) return SELD_EINVAL;
    rc = tconv_addressable(d, o);
    if (rc) return rc;
    const seld_conv_desc m = tconv_mirror(d, o);
    return hc_conv_fwd_out(&m, d->in, dy, w, dx, (hipStream_t)stream);
}

extern "C" size_t seld_hc_conv_transpose_bwd_weight_workspace(const seld_conv_desc* d, const int32_t out_pad[2]) {
    int o[2];
    if (tconv_validate(d, out_pad, o) != SELD_OK || !env().deterministic) return 0;
    return (size_t)d->Cout * d->Cin * d->k[0] * d->k[1] * sizeof(float);
}

// dw[c] += weight gradient of the mirrored convolution with x = dy and dy = x; dbias (nullable) += sum of dy
extern "C" int seld_hc_conv_transpose_bwd_weight_acc(const seld_conv_desc* d, const int32_t out_pad[2], const float* x,
                                                     const float* dy, float* const dw[8], float* dbias, void* workspace,
                                                     size_t workspace_bytes, void* stream) {
    int o[2];
    int rc = tconv_validate(d, out_pad, o);
    if (rc) return rc;
    if (!x || !dy || !dw) return SELD_EINVAL;
    rc = tconv_addressable(d, o);
    if (rc) return rc;
    if (workspace_bytes < seld_hc_conv_transpose_bwd_weight_workspace(d, out_pad)) return SELD_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const seld_conv_desc m = tconv_mirror(d, o);
    rc = hc_wgrad_out(&m, d->in, dy, x, dw, workspace, workspace_bytes, st);
    if (rc) return rc;
    if (dbias) {
        hipLaunchKernelGGL(tconv_bias_grad_kernel, dim3(d->Cout), dim3(256), 0, st, dy, d->N, d->Cout,
                           (long long)o[0] * o[1], dbias);
        rc = check_launch();
    }
    return rc;
}

// Kernel symbol a call would launch: which = 0 forward, 1 input gradient, 2 weight gradient.
extern "C" int seld_hc_conv_transpose_kernel_label(const seld_conv_desc* d, const int32_t out_pad[2], int32_t which,
                                                   char* buf, int32_t buflen) {
    int o[2];
    int rc = tconv_validate(d, out_pad, o);
    if (rc || !buf || buflen < 48) return rc ? rc : SELD_EINVAL;
    if (which == 1 || which == 2) {
        const seld_conv_desc m = tconv_mirror(d, o);
        return seld_hc_conv_kernel_label(&m, which == 1 ? 0 : 2, buf, buflen);
    }
    PgP<2> p{};
    tconv_fill(p, d, o, nullptr);
    const PgCfg c = pg_cfg(p, false);
    snprintf(buf, buflen, "hc_tconv_kernel<%d, %d>", c.ct, c.pt);
    return SELD_OK;
}
