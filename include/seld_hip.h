/*
 * seld_hip.h -- C ABI of the MI355X (gfx950) DualQ-SELD-TCN hot path.
 *
 * The reference (AuroraEchos/Sound-Event-Localization-and-Detection) has no FFI of its own:
 * its seam is the Python call into ATen.  Every entry point below
 * names the reference call it stands in for.  Conventions, all entry points:
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer borrowed for the call;
 *   - tensors are contiguous fp32, NCHW / NCT, hypercomplex components component-major
 *     along the channel axis;
 *   - work is enqueued on `stream` (a hipStream_t passed as void*); nothing synchronises,
 *     nothing allocates (workspaces are caller-provided), nothing throws;
 *   - return value 0 = success, negative = SELD_E* code below.
 */
#ifndef SELD_HIP_H
#define SELD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SELD_OK            0
#define SELD_EINVAL       -1   /* bad descriptor (rank, channel divisibility, groups != 1 ...)      */
#define SELD_EWORKSPACE   -2   /* workspace too small                                              */
#define SELD_ELAUNCH      -3   /* hipLaunch reported an error (see seld_last_hip_error)            */
#define SELD_EUNSUPPORTED -4   /* valid request this build has no kernel for                       */

/* version / capability */
int         seld_abi_version(void);          /* bumps on any signature change                      */
const char* seld_build_arch(void);           /* "gfx950"                                           */
int         seld_last_hip_error(void);       /* last hipError_t seen by a launch in this thread    */
/* The SELD_* environment switches (csrc/env.h: kernel-generation selection, all result-preserving) are read once at
 * first use; seld_env_reload re-reads them. */
int         seld_env_reload(void);

/* ------------------------------------------------------------------------------------------
 * Hypercomplex convolution.  Replaces quaternion_conv (quaternion_ops.py:125-147),
 * dual_quaternion_conv (dual_quaternion_ops.py:111-153) and the real F.conv1d/2d of the
 * domain='R' model (model.py:81-86,106-107,185,198,276).  The kernels read the 1/4/8
 * COMPONENT weight tensors (Cout/A, Cin/A, kh, kw) directly and apply the Hamilton signs
 * while staging into LDS; the expanded (Cout, Cin) matrix never exists in memory.
 * ------------------------------------------------------------------------------------------ */
typedef struct seld_conv_desc {
    int32_t algebra;     /* 1 = real, 4 = quaternion, 8 = dual quaternion                       */
    int32_t ndim;        /* 1 (NCT) or 2 (NCHW); for ndim == 1 use in[0] = k[0] = 1 etc.         */
    int32_t N, Cin, Cout;
    int32_t in[2];       /* input  H, W  (T in in[1] for 1-D)                                   */
    int32_t k[2];        /* kernel kh, kw                                                       */
    int32_t stride[2];
    int32_t pad[2];
    int32_t dil[2];      /* the reference spells the argument `dilatation`                       */
    int32_t groups;      /* 1 for seld_hc_conv_* (the reference never passes anything else);
                            Cin for seld_dwconv_* (depthwise)                                    */
} seld_conv_desc;

/* epilogue flags for seld_hc_conv_fwd_ex */
#define SELD_EPI_NONE        0
#define SELD_EPI_ACCUMULATE  1   /* y += conv(x)   (skip-connection running sum, model.py:210-212) */
#define SELD_EPI_ADD         2   /* y = conv(x) + addend  (x + conv2_residual(y), model.py:132)    */
#define SELD_EPI_STATS       4   /* also accumulate the per-channel sum / sum of squares of the stored result
                                    (BatchNorm batch statistics) into a stats buffer, see below            */

/* Layout of every `stats` buffer: SELD_STATS_REPLICAS rows of 2*C floats [sum(C) | sum of squares(C)];
 * producers add to row (workgroup index % replicas) so that thousands of workgroups do not serialise on
 * 2*C addresses; seld_bn_finalize_ex sums the rows.  The caller zero-fills the buffer before use. */
#define SELD_STATS_REPLICAS 64

int seld_hc_conv_out_shape(const seld_conv_desc* d, int32_t out[2]);

int seld_hc_conv_fwd(const seld_conv_desc* d, const float* x, const float* const w[8],
                     const float* bias /* nullable, (Cout) */, float* y, void* stream);

int seld_hc_conv_fwd_ex(const seld_conv_desc* d, const float* x, const float* const w[8],
                        const float* bias, float* y, int32_t epilogue,
                        const float* addend /* SELD_EPI_ADD */, float* stats /* SELD_EPI_STATS, pre-zeroed */,
                        void* stream);

/* dx = conv_transpose(dy, W)   (autograd of the F.convNd call at quaternion_ops.py:147) */
int seld_hc_conv_bwd_data(const seld_conv_desc* d, const float* dy, const float* const w[8],
                          float* dx, void* stream);
/* Same with a caller-provided workspace of seld_hc_conv_bwd_data_workspace(d) bytes: the component tensors
 * are transposed into it ([c][o][k], one tiny launch) so that the data gradient stages its weight rows
 * with 16-byte loads exactly like the forward (about 2x faster on the TCN layers).  Without (or with too
 * small) a workspace the gather path of seld_hc_conv_bwd_data is used. */
size_t seld_hc_conv_bwd_data_workspace(const seld_conv_desc* d);
int seld_hc_conv_bwd_data_ex(const seld_conv_desc* d, const float* dy, const float* const w[8],
                             float* dx, void* workspace, size_t workspace_bytes, void* stream);

/* seld_hc_conv_bwd_data_ex in two steps: the weight re-layout (Wt[comp][c][o][k] = W[comp][o][c][k], into a workspace of
 * seld_hc_conv_bwd_data_workspace(d) bytes) can be issued ahead of time -- the host mirror does it on a side stream during
 * the forward pass -- and the data gradient then starts from the workspace. */
int seld_hc_conv_transpose_weights(const seld_conv_desc* d, const float* const w[8], void* workspace,
                                   size_t workspace_bytes, void* stream);
int seld_hc_conv_bwd_data_wt(const seld_conv_desc* d, const float* dy, const void* wt_workspace, float* dx, void* stream);

/* dw[c] (component gradients, same shapes as w[c]) and dbias (nullable).  The Hamilton fold
 * (sum of the signed blocks that share a component) is done on device with float atomics, so no
 * workspace is needed any more: seld_hc_conv_bwd_weight_workspace returns 0 and `workspace` may be NULL
 * (both kept for ABI stability). */
size_t seld_hc_conv_bwd_weight_workspace(const seld_conv_desc* d);
int seld_hc_conv_bwd_weight(const seld_conv_desc* d, const float* x, const float* dy,
                            float* const dw[8], float* dbias /* nullable */,
                            void* workspace, size_t workspace_bytes, void* stream);

/* Same, but ACCUMULATES: dw[c] += ..., dbias += ... .  Lets the caller point dw at slices of one flat
 * gradient buffer (zeroed once per step) so that no per-tensor gradient add is ever launched. */
int seld_hc_conv_bwd_weight_acc(const seld_conv_desc* d, const float* x, const float* dy,
                                float* const dw[8], float* dbias /* nullable */, void* stream);

/* ---- two convolutions of one geometry in one launch ------------------------------------------------------
 * A residual block calls the hypercomplex convolution twice on the same tensor with the same geometry:
 * conv1_filter | conv1_gate (model.py:121-122) and conv2_skip | conv2_residual (model.py:130-132).  The pair entry
 * points run both in one launch where that pays (data gradient: ONE kernel sums both contributions, its reduction
 * runs over dyA then dyB; weight gradient: the grid carries both; forward: one launch with two reduction passes per
 * workgroup on the 1x1 layers, two launches of the single kernel otherwise).  The layers are 30-70 us each on an
 * MI355X, so a launch's fixed cost is up to a third of it.
 * seld_hc_conv_pair_supported(d, which) (which: 0 forward, 1 data gradient, 2 weight gradient) tells whether the
 * pair form runs for this shape; if not, the entry point returns SELD_EUNSUPPORTED and the caller issues the two
 * single calls. */
int seld_hc_conv_pair_supported(const seld_conv_desc* d, int32_t which);


int seld_hc_conv_pair_fwd(const seld_conv_desc* d, const float* x, const float* const wA[8], const float* const wB[8],
                          const float* biasA /* nullable */, const float* biasB /* nullable */, float* yA, float* yB,
                          int32_t epilogueA, int32_t epilogueB, const float* addendA /* nullable */,
                          const float* addendB /* nullable */, float* statsA /* nullable */,
                          float* statsB /* nullable */, void* stream);

/* The same from two workspaces filled ahead of time by seld_hc_conv_transpose_weights */
int seld_hc_conv_pair_bwd_data_wt(const seld_conv_desc* d, const float* dyA, const float* dyB, const void* wtA,
                                  const void* wtB, float* dx, void* stream);

/* dx = dgrad(dyA, wA) + dgrad(dyB, wB); workspace: 2 * seld_hc_conv_bwd_data_workspace(d) bytes, required */
int seld_hc_conv_pair_bwd_data(const seld_conv_desc* d, const float* dyA, const float* dyB, const float* const wA[8],
                               const float* const wB[8], float* dx, void* workspace, size_t workspace_bytes,
                               void* stream);

/* dwA[c] += ..., dwB[c] += ..., dbiasA += ..., dbiasB += ... (bias gradients nullable) */
int seld_hc_conv_pair_bwd_weight_acc(const seld_conv_desc* d, const float* x, const float* dyA, const float* dyB,
                                     float* const dwA[8], float* const dwB[8], float* dbiasA, float* dbiasB,
                                     void* stream);

/* Diagnostics: label of the kernel symbol a call would launch ("hc_conv_kernel<4, 4, 1, 3>"), so that
 * HIP-event timings taken by the caller can be matched with rocprofv3's per-kernel statistics.
 * which: 0 forward, 1 data gradient, 2 weight gradient.  buflen >= 48. */
int seld_hc_conv_kernel_label(const seld_conv_desc* d, int32_t which, char* buf, int32_t buflen);

/* ------------------------------------------------------------------------------------------
 * Hypercomplex TRANSPOSED convolution.  Replaces quaternion_transpose_conv (quaternion_ops.py:149-171) and the real
 * F.conv_transpose1d/2d:  y = conv_transpose(x, M, bias, stride, pad, out_pad, dil), M (Cin, Cout, kh, kw) the Hamilton
 * block matrix of the component tensors (Cin/A, Cout/A, kh, kw), as for the forward convolution.  algebra 1 or 4.
 * `d` keeps its layout with TRANSPOSED meaning: Cin / in[] are the transposed convolution's input channels / extent,
 * Cout its output channels.  Output extent per axis: (in - 1)*stride - 2*pad + dil*(k - 1) + out_pad + 1, with
 * out_pad < stride or out_pad < dil (PyTorch's rule).  groups != 1: SELD_EUNSUPPORTED.
 *   seld_hc_conv_transpose_out_shape        the output extent (H, W)
 *   seld_hc_conv_transpose_fwd              y = ... + bias (nullable).  Stride-phase kernel (csrc/hc_conv_transpose.hip):
 *                                           no float atomics, run-to-run bit-identical
 *   seld_hc_conv_transpose_bwd_data         dx = conv(dy, M) with the same stride / pad / dil (the forward convolution)
 *   seld_hc_conv_transpose_bwd_weight_acc   dw[c] += weight gradient, dbias += sum of dy (nullable).  Under
 *                                           SELD_DETERMINISTIC the reproducible path of seld_hc_conv_bwd_weight_det, with a
 *                                           workspace of seld_hc_conv_transpose_bwd_weight_workspace bytes (0 otherwise)
 *   seld_hc_conv_transpose_kernel_label     kernel symbol of a call; which: 0 forward, 1 input gradient, 2 weight gradient */
int seld_hc_conv_transpose_out_shape(const seld_conv_desc* d, const int32_t out_pad[2], int32_t out[2]);
int seld_hc_conv_transpose_fwd(const seld_conv_desc* d, const int32_t out_pad[2], const float* x, const float* const w[8],
                               const float* bias, float* y, void* stream);
int seld_hc_conv_transpose_bwd_data(const seld_conv_desc* d, const int32_t out_pad[2], const float* dy,
                                    const float* const w[8], float* dx, void* stream);
size_t seld_hc_conv_transpose_bwd_weight_workspace(const seld_conv_desc* d, const int32_t out_pad[2]);
int seld_hc_conv_transpose_bwd_weight_acc(const seld_conv_desc* d, const int32_t out_pad[2], const float* x,
                                          const float* dy, float* const dw[8], float* dbias, void* workspace,
                                          size_t workspace_bytes, void* stream);
int seld_hc_conv_transpose_kernel_label(const seld_conv_desc* d, const int32_t out_pad[2], int32_t which, char* buf,
                                        int32_t buflen);

/* ------------------------------------------------------------------------------------------
 * Hypercomplex 3-D convolution and transposed convolution.  Replaces the F.conv3d / F.conv_transpose3d calls of
 * quaternion_conv / dual_quaternion_conv / quaternion_transpose_conv (quaternion_ops.py:125-171,
 * dual_quaternion_ops.py:111-153) for 5-D input (N, C, D, H, W).  Component tensors (Cout/A, Cin/A, kd, kh, kw) for the
 * convolution, (Cin/A, Cout/A, kd, kh, kw) for the transposed one; per-axis arrays are (D, H, W).  The transposed
 * entry points take `d` with transposed meaning as seld_hc_conv_transpose_* does, algebra 1 or 4, and out_pad[3] under
 * PyTorch's rule (out_pad < stride or out_pad < dil).  Refused: groups != 1, a stride above 16, and extents whose
 * images or weights outgrow the kernels' 32-bit offsets (SELD_EUNSUPPORTED); malformed descriptors (SELD_EINVAL).
 * Nothing is launched or written on refusal.
 *   *_out_shape               the output extent (D, H, W)
 *   *_fwd                     y = ... + bias (nullable).  Convolution: implicit-GEMM kernel; transposed: stride-phase
 *                             kernel (csrc/hc_conv3d.hip)
 *   *_bwd_data                dx: the other of the two kernels, cut to the input extent
 *   *_bwd_weight_workspace    bytes of the workspace *_bwd_weight_acc needs (never 0 for a valid descriptor)
 *   *_bwd_weight_acc          dw[c] += weight gradient, dbias (nullable) += channel sums of dy: per-split partials in
 *                             the workspace, then one fixed-order fold onto the components
 *   *_kernel_label            kernel symbol of a call; which: 0 forward, 1 input gradient, 2 weight gradient
 * No float atomics: every call is run-to-run bit-identical, with or without SELD_DETERMINISTIC. */
typedef struct seld_conv3d_desc {
    int32_t algebra, N, Cin, Cout;
    int32_t in[3], k[3], stride[3], pad[3], dil[3];
    int32_t groups;
} seld_conv3d_desc;

int seld_hc_conv3d_out_shape(const seld_conv3d_desc* d, int32_t out[3]);
int seld_hc_conv3d_fwd(const seld_conv3d_desc* d, const float* x, const float* const w[8], const float* bias, float* y,
                       void* stream);
int seld_hc_conv3d_bwd_data(const seld_conv3d_desc* d, const float* dy, const float* const w[8], float* dx, void* stream);
size_t seld_hc_conv3d_bwd_weight_workspace(const seld_conv3d_desc* d);
int seld_hc_conv3d_bwd_weight_acc(const seld_conv3d_desc* d, const float* x, const float* dy, float* const dw[8],
                                  float* dbias, void* workspace, size_t workspace_bytes, void* stream);
int seld_hc_conv3d_kernel_label(const seld_conv3d_desc* d, int32_t which, char* buf, int32_t buflen);

int seld_hc_conv3d_transpose_out_shape(const seld_conv3d_desc* d, const int32_t out_pad[3], int32_t out[3]);
int seld_hc_conv3d_transpose_fwd(const seld_conv3d_desc* d, const int32_t out_pad[3], const float* x,
                                 const float* const w[8], const float* bias, float* y, void* stream);
int seld_hc_conv3d_transpose_bwd_data(const seld_conv3d_desc* d, const int32_t out_pad[3], const float* dy,
                                      const float* const w[8], float* dx, void* stream);
size_t seld_hc_conv3d_transpose_bwd_weight_workspace(const seld_conv3d_desc* d, const int32_t out_pad[3]);
int seld_hc_conv3d_transpose_bwd_weight_acc(const seld_conv3d_desc* d, const int32_t out_pad[3], const float* x,
                                            const float* dy, float* const dw[8], float* dbias, void* workspace,
                                            size_t workspace_bytes, void* stream);
int seld_hc_conv3d_transpose_kernel_label(const seld_conv3d_desc* d, const int32_t out_pad[3], int32_t which, char* buf,
                                          int32_t buflen);

/* ------------------------------------------------------------------------------------------
 * Depthwise convolution: the `depthwise` nn.Conv1d / nn.Conv2d(in, in, k, stride, padding, groups=in) of
 * DepthwiseSeparableConv1D / DepthwiseSeparableConv2D (dual_quaternion_layers.py:19-47), and torch's groups == Cin with
 * any channel multiplier m: output channel o reads input channel o / m.  Descriptor: seld_conv_desc with algebra 1,
 * groups = Cin, Cout = m * Cin; weight (Cout, 1, kh, kw) contiguous, any kh * kw <= 255, stride, zero padding and
 * dilation.  Exact fp32 VALU kernels (csrc/dwconv.hip).  SELD_EINVAL: groups != Cin, Cout % Cin != 0, algebra != 1,
 * non-positive sizes, an empty output, missing buffers; SELD_EUNSUPPORTED: kh * kw > 255 or an image of either operand of
 * 2^28 elements or more; SELD_EWORKSPACE: workspace too small.  Nothing is launched or written on refusal.
 *   seld_dwconv_out_shape              output extent (H, W) (H = 1 for ndim 1)
 *   seld_dwconv_fwd                    y = dwconv(x, w) + bias (nullable)
 *   seld_dwconv_bwd_data               dx = dwconv^T(dy, w): gather form, no atomics
 *   seld_dwconv_bwd_weight_workspace   bytes *_bwd_weight_acc needs (0 for a refused descriptor)
 *   seld_dwconv_bwd_weight_acc         dw += sum x * dy, dbias (nullable) += sum dy: per-tile partials of every tap in
 *                                      the workspace, then one fixed-order fold
 *   seld_dwconv_kernel_label           kernel symbol of a call; which: 0 forward, 1 input gradient, 2 weight gradient
 * No float atomics: every call is run-to-run bit-identical, with or without SELD_DETERMINISTIC. */
int seld_dwconv_out_shape(const seld_conv_desc* d, int32_t out[2]);
int seld_dwconv_fwd(const seld_conv_desc* d, const float* x, const float* w, const float* bias, float* y, void* stream);
int seld_dwconv_bwd_data(const seld_conv_desc* d, const float* dy, const float* w, float* dx, void* stream);
size_t seld_dwconv_bwd_weight_workspace(const seld_conv_desc* d);
int seld_dwconv_bwd_weight_acc(const seld_conv_desc* d, const float* x, const float* dy, float* dw, float* dbias,
                               void* workspace, size_t workspace_bytes, void* stream);
int seld_dwconv_kernel_label(const seld_conv_desc* d, int32_t which, char* buf, int32_t buflen);

/* ------------------------------------------------------------------------------------------
 * Element-wise quaternion algebra (csrc/quat_algebra.hip): get_modulus / get_normalized / hamilton_product of
 * quaternion_ops.py:102-122, :467-506 and dual_quaternion_ops.py:88-108, :374-412, q_normalize / quaternion_exp of
 * dual_quaternion_ops.py:206-243.  Exact fp32 VALU kernels, one pass over memory each (the sums over dim 0: one pass
 * and a fold), forward and first derivatives.
 * seld_quat_shape: the contiguous input as (dim0, mid, comp, inner), `comp` the component axis [r | i | j | k]:
 *   2-D (N, 4Q)      -> (N, 1, 4Q, 1)        3-D (B, T, 4Q)          -> (B, T, 4Q, 1)
 *   4-D (N, 4Q, H, W) -> (N, 1, 4Q, H*W)     5-D (N, 4Q, D, H, W)    -> (N, 1, 4Q, D*H*W)
 * With Q = comp / 4 and M = Q * inner, per-quaternion arrays are (dim0, mid, M) and arrays summed over dim 0 (mid, M).
 * layout (q_normalize / quaternion_exp, which concatenate on dim 1 whatever the rank): SELD_QUAT_LAYOUT_INPUT: y and dy
 * laid out like x; SELD_QUAT_LAYOUT_CAT1: y and dy are (dim0, 4, mid, M), i.e. (B, 4T, Q) for a 3-D input, written and
 * read in place (no permuted copy).  The two coincide for mid == 1.
 * SELD_EINVAL: comp % 4 != 0, a non-positive extent, an unknown layout, a NULL pointer; SELD_EUNSUPPORTED: 2^31
 * quaternions or more; SELD_EWORKSPACE: workspace missing or smaller than seld_quat_reduce_workspace(shape).  Nothing
 * is launched or written on refusal.  16-byte accesses when M % 4 == 0 and every pointer is 16-byte aligned.
 *   seld_quat_modulus_fwd         y[dim0, mid, M] = sqrt(r^2 + i^2 + j^2 + k^2)            (vector_form=True)
 *   seld_quat_modulus_bwd         dx_c = dy * x_c / |q|   (0 at |q| = 0, where the reference's autograd gives NaN)
 *   seld_quat_reduce_workspace    bytes the three calls below with a workspace need (0 for a refused shape)
 *   seld_quat_modulus_sum_fwd     y[mid, M] = sqrt(sum over dim0 of r^2 + i^2 + j^2 + k^2)  (vector_form=False)
 *   seld_quat_modulus_sum_bwd     dx_c = dy[mid, M] * x_c / y[mid, M]   (0 where y = 0)
 *   seld_quat_normalized_fwd      y_c = x_c / (modulus[mid, M] + eps), modulus from seld_quat_modulus_sum_fwd
 *   seld_quat_normalized_bwd      dx_c = dy_c / (D + eps) - x_c * G / ((D + eps)^2 * D), D = modulus, G[mid, M] the sum
 *                                 over dim0 and the components of dy * x (second term dropped where D = 0)
 *   seld_quat_normalize_fwd/_bwd  q_normalize: y_c = x_c / sqrt(|q|^2 + 1e-4); finite everywhere (dx = 100 dy at q = 0)
 *   seld_quat_exp_fwd/_bwd        quaternion_exp: n = |(i, j, k)| + 1e-4, y = exp(r) [cos n, (i, j, k) sin(n) / n]; at
 *                                 i = j = k = 0 the gradient is d/dr = the result's, d/d(i, j, k) = exp(r) dy sin(n) / n
 *                                 (the reference's autograd gives NaN there)
 *   seld_quat_hamilton_fwd        y = q0 (x) q1, both of `shape`
 *   seld_quat_hamilton_bwd        dq0 = dy (x) conj(q1) and dq1 = conj(q0) (x) dy from one read of q0, q1, dy
 * Sums over dim 0 are per-slice partials in the workspace and one fixed-order fold; no float atomics: every call is
 * run-to-run bit-identical, with or without SELD_DETERMINISTIC. */
typedef struct {
    int32_t dim0;        /* extent of dim 0: what the summed forms reduce over                                   */
    int32_t mid;         /* T of a 3-D input (B, T, 4Q), else 1                                                   */
    int32_t comp;        /* extent of the component axis, 4Q                                                      */
    int32_t inner;       /* product of the extents after the component axis (1 for 2-D / 3-D input)               */
} seld_quat_shape;
#define SELD_QUAT_LAYOUT_INPUT  0
#define SELD_QUAT_LAYOUT_CAT1   1
int seld_quat_modulus_fwd(const seld_quat_shape* shape, const float* x, float* y, void* stream);
int seld_quat_modulus_bwd(const seld_quat_shape* shape, const float* x, const float* dy, float* dx, void* stream);
size_t seld_quat_reduce_workspace(const seld_quat_shape* shape);
int seld_quat_modulus_sum_fwd(const seld_quat_shape* shape, const float* x, float* y, void* workspace,
                              size_t workspace_bytes, void* stream);
int seld_quat_modulus_sum_bwd(const seld_quat_shape* shape, const float* x, const float* y, const float* dy, float* dx,
                              void* stream);
int seld_quat_normalized_fwd(const seld_quat_shape* shape, const float* x, const float* modulus, float eps, float* y,
                             void* stream);
int seld_quat_normalized_bwd(const seld_quat_shape* shape, const float* x, const float* modulus, const float* dy, float eps,
                             float* dx, void* workspace, size_t workspace_bytes, void* stream);
int seld_quat_normalize_fwd(const seld_quat_shape* shape, int32_t layout, const float* x, float* y, void* stream);
int seld_quat_normalize_bwd(const seld_quat_shape* shape, int32_t layout, const float* x, const float* dy, float* dx,
                            void* stream);
int seld_quat_exp_fwd(const seld_quat_shape* shape, int32_t layout, const float* x, float* y, void* stream);
int seld_quat_exp_bwd(const seld_quat_shape* shape, int32_t layout, const float* x, const float* dy, float* dx,
                      void* stream);
int seld_quat_hamilton_fwd(const seld_quat_shape* shape, const float* q0, const float* q1, float* y, void* stream);
int seld_quat_hamilton_bwd(const seld_quat_shape* shape, const float* q0, const float* q1, const float* dy, float* dq0,
                           float* dq1, void* stream);

/* ------------------------------------------------------------------------------------------
 * Quaternion ROTATION weight: quaternion_conv_rotation / quaternion_transpose_conv_rotation / quaternion_linear_rotation
 * (quaternion_ops.py:174-388) build one real weight K from the component tensors (A, B, *taps) element by element and run
 * one real convolution / transposed convolution / matmul with it (the algebra-1 entry points above and below).
 * Per element, with u = (r, i, j, k), n = |u|, f = 2n:  E = I + f*Q(u),  Q the 3x3 rotation quadratic of
 * csrc/quat_rotation.hip;  K[m*A + a][c*B + b][t] = E[m][c](a, b, t), K (3A, 3B, *taps).  qformat (quaternion_format):
 * K (4A, 4B, *taps), block row 0 and block column 0 zero, E at block (m+1, c+1).
 *   layout SELD_ROT_LAYOUT_CONV    K as above (F.convNd / F.conv_transposeNd weight)
 *   layout SELD_ROT_LAYOUT_LINEAR  K^T, (MB*B, MB*A) with MB = 3 or 4, taps == 1 (the SELD_LIN_REAL weight)
 *   seld_quat_rotation_form        writes all of K, zero blocks included
 *   seld_quat_rotation_form_bwd    dw[c] (+)= dL/du_c from dK (accumulate 0: store, 1: add); no atomics, run-to-run
 *                                  bit-identical.  n = 0 gives inf / NaN, as the reference's autograd.
 * SELD_EINVAL: bad layout / sizes (A, B, taps >= 1), taps != 1 with the linear layout, NULL pointers. */
#define SELD_ROT_LAYOUT_CONV    0
#define SELD_ROT_LAYOUT_LINEAR  1
int seld_quat_rotation_form(int32_t layout, int32_t qformat, int32_t A, int32_t B, int32_t taps,
                            const float* const w[4], float* K, void* stream);
int seld_quat_rotation_form_bwd(int32_t layout, int32_t qformat, int32_t A, int32_t B, int32_t taps,
                                const float* const w[4], const float* dK, float* const dw[4], int32_t accumulate,
                                void* stream);

/* ------------------------------------------------------------------------------------------
 * Hypercomplex / real linear  y[rows, out] = x[rows, in] @ M + b.
 *   SELD_LIN_REAL   : torch.nn.Linear, weight (out, in)                 (model.py:23,439,454,458)
 *   SELD_LIN_QUAT   : quaternion_linear, weights (in/4, out/4)          (quaternion_ops.py:299-327)
 *   SELD_LIN_DUALQ  : dual_quaternion_linear, weights (in/8, out/8), the TRANSPOSED block
 *                     arrangement of dual_quaternion_ops.py:170-188
 * ------------------------------------------------------------------------------------------ */
#define SELD_LIN_REAL   1
#define SELD_LIN_QUAT   4
#define SELD_LIN_DUALQ  8

int seld_hc_linear_fwd(int32_t kind, int32_t rows, int32_t in_features, int32_t out_features,
                       const float* x, const float* const w[8], const float* bias, float* y, void* stream);
/* dx = dy @ M^T (nullable), dw[c] = folded x^T @ dy (nullable), dbias = column sums of dy (nullable).
 * workspace: seld_hc_linear_bwd_workspace bytes (up to 8 row splits of x^T @ dy and of the column sums, written with
 * plain stores and added in a fixed order by the fold: nothing is zeroed, no atomics, run-to-run identical). */
size_t seld_hc_linear_bwd_workspace(int32_t kind, int32_t in_features, int32_t out_features);
int seld_hc_linear_bwd(int32_t kind, int32_t rows, int32_t in_features, int32_t out_features,
                       const float* x, const float* dy, const float* const w[8],
                       float* dx /* nullable */, float* const dw[8] /* nullable */, float* dbias /* nullable */,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * BatchNorm (torch.nn.BatchNorm1d/2d at model.py:88-92,279; eps 1e-5, momentum 0.1) fused
 * with the activation that follows it in the reference graph.
 * x is (N, C, S) with S = prod(spatial).
 * ------------------------------------------------------------------------------------------ */
#define SELD_ACT_NONE    0
#define SELD_ACT_RELU    1
#define SELD_ACT_TANH    2
#define SELD_ACT_SIGMOID 3

/* per-channel sum / sum of squares of x (N, C, S) into a stats buffer (layout above) */
int seld_channel_stats(const float* x, int32_t N, int32_t C, int32_t S, float* stats, void* stream);

/* from raw sums: mean/invstd (saved for backward) and the running-stat update (train mode), plus the rest of
 * torch.nn.BatchNorm's train-mode bookkeeping in the one launch: *num_batches_tracked += 1 (nullable;
 * `_BatchNorm.forward` does it as a separate op) and, if clear_stats != 0, the stats buffer is left zero-filled so that
 * the caller can reuse it without another fill. */
int seld_bn_finalize_ex(float* stats, int32_t C, int64_t count, float eps, float momentum,
                        float* mean, float* invstd, float* running_mean /* nullable */,
                        float* running_var /* nullable */, int64_t* num_batches_tracked /* nullable */,
                        int32_t clear_stats, void* stream);

/* two BatchNorm layers of the same channel count in one launch (batch_filter2 / batch_gate2 of a residual block,
 * model.py:123-126, whose statistics the one filter|gate pair convolution gathered) */
int seld_bn_finalize2_ex(float* statsA, float* statsB, int32_t C, int64_t count, float eps, float momentum,
                         float* meanA, float* invstdA, float* running_meanA, float* running_varA,
                         int64_t* num_batches_trackedA, float* meanB, float* invstdB, float* running_meanB,
                         float* running_varB, int64_t* num_batches_trackedB, int32_t clear_stats, void* stream);

/* eval mode: mean = running_mean, invstd = 1/sqrt(running_var + eps) */
int seld_bn_eval_stats(const float* running_mean, const float* running_var, int32_t C, float eps,
                       float* mean, float* invstd, void* stream);

/* BatchNorm2d -> ReLU -> MaxPool2d(ph, pw) (stride = window, floor mode) in one pass (model.py:278-281):
 * reads the conv output y (N, C, H, W), writes the pooled map and a uint8 arg-max per pooled element. */
int seld_bn_relu_pool_fwd(const float* y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t ph, int32_t pw,
                          const float* mean, const float* invstd, const float* gamma, const float* beta,
                          float* pooled, uint8_t* idx, void* stream);
/* Backward of the above: red (2C, pre-zeroed) receives dgamma | dbeta (reduced from pooled-size tensors
 * only), dy (N, C, H, W) the gradient w.r.t. the conv output.  train = 0: running statistics were used. */
int seld_bn_relu_pool_bwd(const float* dpooled, const float* pooled, const uint8_t* idx, const float* y,
                          int32_t N, int32_t C, int32_t H, int32_t W, int32_t ph, int32_t pw, const float* mean,
                          const float* invstd, const float* gamma, const float* beta, int32_t train,
                          float* red, float* dy, void* stream);
/* The stage's Dropout (model.py:282) in the same passes, for the shapes seld_bn_relu_pool_drop_ok accepts (pw == 1,
 * W % 4 == 0, H % ph == 0): forward also writes dropped = pooled * mask (the mask seld_dropout_fwd draws for the same
 * seed / offset / state on the pooled tensor); backward takes dpooled = the gradient BEHIND the Dropout and replays the
 * mask while it loads it.  drop_p == 0: identical to the two entries above (dropped is not written). */
int seld_bn_relu_pool_drop_ok(int32_t H, int32_t W, int32_t ph, int32_t pw);
int seld_bn_relu_pool_fwd_drop(const float* y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t ph, int32_t pw,
                               const float* mean, const float* invstd, const float* gamma, const float* beta,
                               float* pooled, uint8_t* idx, float drop_p, uint64_t seed, uint64_t offset,
                               const uint64_t* state, float* dropped, void* stream);
int seld_bn_relu_pool_bwd_drop(const float* dpooled, const float* pooled, const uint8_t* idx, const float* y,
                               int32_t N, int32_t C, int32_t H, int32_t W, int32_t ph, int32_t pw, const float* mean,
                               const float* invstd, const float* gamma, const float* beta, int32_t train,
                               float* red, float* dy, float drop_p, uint64_t seed, uint64_t offset,
                               const uint64_t* state, void* stream);

/* The same backward for a convolution whose INPUT needs no gradient (the first layer), without ever writing the
 * gradient w.r.t. the conv output (1.6 GB at batch 32):
 *   seld_bn_relu_pool_bwd_coef        : the reductions (red = dgamma | dbeta) and coef = [c1 | a | c0] (3C) such that
 *                                       dy = y*c1 + dz*a + c0; conv_dbias (nullable, C) += sum over positions of dy
 *   seld_hc_conv_bwd_weight_bnpool_acc: dw[c] += weight gradient, dy formed from y / pooled / dpooled / idx / coef while
 *                                       the operand is staged (3x3 taps, pooling along H only; else SELD_EUNSUPPORTED) */
int seld_bn_relu_pool_bwd_coef(const float* dpooled, const float* pooled, const uint8_t* idx, const float* y,
                               int32_t N, int32_t C, int32_t H, int32_t W, int32_t ph, int32_t pw, const float* mean,
                               const float* invstd, const float* gamma, const float* beta, int32_t train,
                               float* red, float* coef, float* conv_dbias /* nullable */, void* stream);
/* the same with dpooled = the gradient BEHIND the stage's Dropout(drop_p) (model.py:282): its mask -- the one
 * seld_dropout_fwd draws for (seed, offset, state) -- is replayed while dpooled is loaded, no dropout-backward pass */
int seld_bn_relu_pool_bwd_coef_drop(const float* dpooled, const float* pooled, const uint8_t* idx, const float* y,
                                    int32_t N, int32_t C, int32_t H, int32_t W, int32_t ph, int32_t pw,
                                    const float* mean, const float* invstd, const float* gamma, const float* beta,
                                    int32_t train, float* red, float* coef, float* conv_dbias, float drop_p,
                                    uint64_t seed, uint64_t offset, const uint64_t* state, void* stream);
int seld_hc_conv_bwd_weight_bnpool_acc(const seld_conv_desc* d, const float* x, const float* y, const float* pooled,
                                       const float* dpooled, const uint8_t* idx, int32_t ph, const float* coef,
                                       float* const dw[8], void* stream);
int seld_hc_conv_bwd_weight_bnpool_drop_acc(const seld_conv_desc* desc, const float* x, const float* y,
                                            const float* pooled, const float* dpooled, const uint8_t* idx, int32_t ph,
                                            const float* coef, float* const dw[8], float drop_p, uint64_t seed,
                                            uint64_t offset, const uint64_t* state, void* stream);

/* y = act(gamma * (x - mean) * invstd + beta) */
int seld_bn_act_fwd(const float* x, int32_t N, int32_t C, int32_t S, const float* mean, const float* invstd,
                    const float* gamma, const float* beta, int32_t act, float* y, void* stream);

/* backward of the above in two passes:
 *   reduce: dgamma[c] = sum dz * xhat, dbeta[c] = sum dz, with dz = dy * act'(y)
 *   apply : dx = gamma * invstd * (dz - dbeta/M - xhat * dgamma/M)   (train: batch statistics)
 *           dx = gamma * invstd * dz                                  (eval: running statistics) */
int seld_bn_act_bwd_reduce(const float* dy, const float* x, const float* y, int32_t N, int32_t C, int32_t S,
                           const float* mean, const float* invstd, const float* gamma, const float* beta,
                           int32_t act, float* dgamma_dbeta /* (2C) pre-zeroed */, void* stream);
int seld_bn_act_bwd_apply(const float* dy, const float* x, const float* y, int32_t N, int32_t C, int32_t S,
                          const float* mean, const float* invstd, const float* gamma, const float* beta,
                          int32_t act, const float* dgamma_dbeta, int32_t train, float* dx, void* stream);

/* One-pass training-mode backward of the same op: dgamma / dbeta are ADDED to dgamma_dbeta (it need not be zero),
 * dx = BatchNorm-backward((dy [+ dy2]) * act'(y))  (dx nullable: parameter gradients only; dy2 nullable: the gradient
 * from y's second consumer -- the residual sum x_hat + conv2_residual(..) of model.py:132 -- added on load instead of
 * by a separate kernel).  SELD_EUNSUPPORTED when S % 4 != 0 or N*S > SELD_BN_ONE_PASS_MAX: use the reduce + apply
 * pair. */
#define SELD_BN_ONE_PASS_MAX 32768
int seld_bn_act_bwd_fused(const float* dy, const float* x, const float* y, int32_t N, int32_t C, int32_t S,
                          const float* mean, const float* invstd, const float* gamma, int32_t act,
                          float* dgamma_dbeta, const float* dy2, float* dx, void* stream);

/* gated activation of the residual block (model.py:121-128):
 *   y = tanh(bn_f(yf)) * sigmoid(bn_g(yg)) * mask[n, c]      (mask nullable = Dropout1d channel mask,
 *                                                            already scaled by 1/(1-p))            */
int seld_gate_fwd(const float* yf, const float* yg, int32_t N, int32_t C, int32_t S,
                  const float* mean_f, const float* invstd_f, const float* gamma_f, const float* beta_f,
                  const float* mean_g, const float* invstd_g, const float* gamma_g, const float* beta_g,
                  const float* mask, float* y, void* stream);
/* backward: reduce pass accumulates (dgamma_f, dbeta_f, dgamma_g, dbeta_g) into red[4C] (pre-zeroed),
 * apply pass writes dyf, dyg */
int seld_gate_bwd_reduce(const float* dy, const float* yf, const float* yg, int32_t N, int32_t C, int32_t S,
                         const float* mean_f, const float* invstd_f, const float* gamma_f, const float* beta_f,
                         const float* mean_g, const float* invstd_g, const float* gamma_g, const float* beta_g,
                         const float* mask, float* red, void* stream);
int seld_gate_bwd_apply(const float* dy, const float* yf, const float* yg, int32_t N, int32_t C, int32_t S,
                        const float* mean_f, const float* invstd_f, const float* gamma_f, const float* beta_f,
                        const float* mean_g, const float* invstd_g, const float* gamma_g, const float* beta_g,
                        const float* mask, const float* red, int32_t train, float* dyf, float* dyg, void* stream);

/* First stage with the pooling decision inside the convolution (csrc/hcq_first.hip hcq_first_pool_kernel): for
 * conv -> BatchNorm2d -> ReLU -> MaxPool2d(8, 1) on the network input (model.py:273-281) the sign of gamma says whether a
 * window's maximum after BatchNorm + ReLU sits at the largest or the smallest conv output, so the convolution writes y,
 * the batch statistics and, per window, that raw value and its row; seld_bn_pool_finish applies relu(a v + b) on the
 * pooled-size tensor once the statistics are final.  wpack = seld_hcq_pack(desc, mode 2, ...); SELD_EUNSUPPORTED unless
 * seld_hcq_pack_floats(desc, 2, 1) > 0 (3x3 'same', 1-2 input block channels, height % 8 == 0, width % 64 == 0). */
int seld_hcq_first_pool(const seld_conv_desc* desc, const float* x, const float* wpack, const float* bias,
                        const float* gamma, int32_t want_stats, float* y, float* stats, float* pool_raw, uint8_t* idx,
                        void* stream);
/* The same pooling convolution when BatchNorm's statistics are known BEFORE it runs (seld_first_stage_bn): no y, no
 * statistics, and BatchNorm + ReLU + the stage's Dropout (model.py:279-282) are applied to the window value in the
 * epilogue: out = Dropout(relu(a raw + b)) with the mask seld_dropout_fwd draws for (seed, offset, state) on `out`
 * (drop_p = 0: none).  idx as above; pool_raw (same size, must be allocated) is written ONLY for channels with
 * gamma == 0 -- the one case in which seld_first_stage_bwd cannot recover xhat from out. */
int seld_hcq_first_pool_bn(const seld_conv_desc* desc, const float* x, const float* wpack, const float* bias,
                           const float* gamma, const float* beta, const float* mean, const float* invstd,
                           float drop_p, uint64_t seed, uint64_t offset, const uint64_t* state, float* pool_raw,
                           uint8_t* idx, float* out, void* stream);
/* out (nullable) = Dropout(p)(pooled) in the same pass, the mask seld_dropout_fwd would draw for (seed, offset, state) */
/* ------------------------------------------------------------------------------------------
 * First stage without its convolution output (csrc/first_stage.hip): conv3x3 on the 8-channel network input ->
 * BatchNorm2d (batch statistics) -> ReLU -> MaxPool2d(8, 1) -> Dropout, model.py:273-283.  The convolution is linear in
 * the input, so BatchNorm's statistics follow from the input's second moments (gram: 80 x 80 doubles, [G; s], count at
 * [72][72]) and the weights, and the backward pass needs the pooled-size tensors and x only.
 *   forward : seld_first_stage_gram -> seld_first_stage_bn (mean, invstd, running statistics, W G) ->
 *             seld_hcq_first_pool_bn (the stage's output + window row; three launches + two small folds in all)
 *   backward: seld_first_stage_bwd (dgamma, dbeta, component weight gradients; reproducible: no atomics)
 * Shapes: Cin = 8, 3x3 'same' stride 1, H % 8 == 0, W % 64 == 0 (backward: Cout in {64, 128, 192}; 64 only for algebra 1 / 4); workspace queries
 * return 0 otherwise. */
size_t seld_first_stage_gram_workspace(const seld_conv_desc* desc);
int seld_first_stage_gram(const seld_conv_desc* desc, const float* x, void* workspace, size_t workspace_bytes, void* stream);
int seld_first_stage_bn(const seld_conv_desc* desc, const float* const w[8], const float* bias, const double* gram, float eps,
                        float momentum, float* mean, float* invstd, float* running_mean, float* running_var,
                        int64_t* num_batches_tracked, float* wg /* (Cout, 72) or NULL */, void* stream);
size_t seld_first_stage_bwd_workspace(const seld_conv_desc* desc);
int seld_first_stage_bwd(const seld_conv_desc* desc, const float* x, const float* dout, const float* out, const float* raw,
                         const uint8_t* idx, const float* mean, const float* invstd, const float* gamma, const float* beta,
                         const float* bias, const double* gram, const float* wg, float* dgamma, float* dbeta,
                         float* const dw[8], float drop_p, void* workspace, size_t workspace_bytes, void* stream);

int seld_bn_pool_finish(const float* raw, int32_t N, int32_t C, int32_t S /* pooled H * W */, const float* mean,
                        const float* invstd, const float* gamma, const float* beta, float* pooled, float p, uint64_t seed,
                        uint64_t offset, const uint64_t* state, float* out, void* stream);

/* One-pass training-mode backward of the gate (adds into red[4C]; SELD_EUNSUPPORTED when S % 4 != 0 or
 * N*S > SELD_GATE_ONE_PASS_MAX). */
#define SELD_GATE_ONE_PASS_MAX 16384
int seld_gate_bwd_fused(const float* dy, const float* yf, const float* yg, int32_t N, int32_t C, int32_t S,
                        const float* mean_f, const float* invstd_f, const float* gamma_f, const float* beta_f,
                        const float* mean_g, const float* invstd_g, const float* gamma_g, const float* beta_g,
                        const float* mask, float* red, float* dyf, float* dyg, void* stream);

/* Diagnostics: the kernel an entry point above launches for (N, C, S) under the current switches, answered by the
 * selection code the entry point itself runs: "bn_act_bwd_channel_kernel<4>", "gate_bwd_reduce_row_kernel",
 * "bn_act_bwd_reduce_kernel[x4, 2 chunks]" (x4 / x1: 16-byte or single-element walk; chunks: workgroups per channel
 * that add into the result, 1 under SELD_DETERMINISTIC).  SELD_EUNSUPPORTED where the fused entry point answers so.
 * buflen >= 48. */
#define SELD_NORM_BN_BWD_FUSED    0
#define SELD_NORM_BN_BWD_REDUCE   1
#define SELD_NORM_BN_BWD_APPLY    2
#define SELD_NORM_GATE_FWD        3
#define SELD_NORM_GATE_BWD_FUSED  4
#define SELD_NORM_GATE_BWD_REDUCE 5
#define SELD_NORM_GATE_BWD_APPLY  6
int seld_norm_kernel_label(int32_t op, int32_t N, int32_t C, int32_t S, char* buf, int32_t buflen);

/* ------------------------------------------------------------------------------------------
 * Quaternion / dual-quaternion convolution by the 8-multiplication Hamilton product (csrc/hcq_conv.hip).
 * Same mathematics as seld_hc_conv_fwd / _bwd_data (quaternion_ops.py:125-147, dual_quaternion_ops.py:111-153):
 * the bilinear map w (x) x has rank 8, so the convolution is evaluated as 8 real GEMMs of a quarter of the K extent
 * on sums of two components (3 x 8 = 24 sub-products for the dual quaternion instead of 48) and the results
 * recombined in the epilogue; fp32 results differ from the block-matrix evaluation by rounding only.
 * Takes 'same' stride-1 convolutions with 1x1, 1x3 (any dilation) or 3x3 taps, row length a multiple of 64,
 * algebra 4 or 8, Cout/A a multiple of 16 (dual quaternion also 24).
 *   seld_hcq_pack_floats  size of the packed weight-form buffer (0: shape not taken, use seld_hc_conv_*)
 *   seld_hcq_pack         weight forms in MFMA fragment order, once per optimiser step and direction
 *                         (mode 0 forward, 1 data gradient); npair = 2 packs two convolutions of the same input
 *                         (conv1_filter | conv1_gate, conv2_skip | conv2_residual, model.py:121-132) for one launch:
 *                         two outputs (forward) or the sum of the two data gradients (mode 1)
 *   seld_hcq_conv         y[s] = W_s (x) x [+ bias][+ addend][statistics]  (mode 0), dx = data gradient (mode 1, x = dy)
 * ------------------------------------------------------------------------------------------ */
size_t seld_hcq_pack_floats(const seld_conv_desc* desc, int32_t mode, int32_t npair);
int seld_hcq_pack(const seld_conv_desc* desc, int32_t mode, int32_t npair, const float* const wA[8],
                  const float* const wB[8], float* wpack, void* stream);
/* mode 0: y[s] = W_s (x) x for s < npair.  mode 1: y[0] = dgrad(x, W_A) [+ dgrad(x2, W_B) if npair == 2]. */
int seld_hcq_conv(const seld_conv_desc* desc, int32_t mode, int32_t npair, const float* x, const float* x2,
                  const float* wpack, float* const y[2], const float* const bias[2], const int32_t epilogue[2],
                  const float* const addend[2], float* const stats[2], void* stream);
int seld_hcq_kernel_label(const seld_conv_desc* desc, int32_t mode, int32_t npair, char* buf, int32_t buflen);
/* Host-only: the launch behind that label -- out = grid x, grid y, dynamic LDS bytes, byte offset of the fragment ring in
 * LDS and its slot kind (1: half pairs; both 0 without a ring), image rows per workgroup (0: not a first-layer kernel).
 * mode 2: the launch of seld_hcq_first_pool. */
int seld_hcq_launch_shape(const seld_conv_desc* desc, int32_t mode, int32_t npair, int32_t out[6]);
/* Every layer's weight forms in ONE launch per optimiser step: the caller builds a table of entries
 * (seld_hcq_pack_entry fills one entry of seld_hcq_pack_entry_bytes() bytes in host memory), copies it to the device
 * once, and calls seld_hcq_pack_flat after every weight update: starts_dev[e] = first 256-float block of entry e (prefix
 * sums of ceil(floats_e / 256)), starts_dev[nentries] = total_blocks. */
size_t seld_hcq_pack_entry_bytes(void);
int seld_hcq_pack_entry(const seld_conv_desc* desc, int32_t mode, int32_t npair, const float* const wA[8],
                        const float* const wB[8], float* wpack, void* entry_host);
int seld_hcq_pack_flat(const void* table_dev, const int32_t* starts_dev, int32_t nentries, int32_t total_blocks,
                       void* stream);

/* Weight gradient of the quaternion layers on the fast product (csrc/hcq_wgrad.hip): dW = sum over positions of
 * dy (x) conj(x) is again a Hamilton product per (output block channel, input block channel, tap): 8 real sub-products
 * instead of 16.  (Dual quaternion: seld_hcq_wgrad_group, or seld_hc_conv_bwd_weight_acc.)  dwA[c] += gradient of
 * conv(x; W_A) given dyA; npair == 2: also dwB[c] += that of a second convolution of the same input given dyB
 * (conv1_filter | conv1_gate, conv2_skip | conv2_residual).  Accumulating (the
 * caller's buffers are FlatAdam's gradient slices, train.py:557); no bias gradient (use seld_hc_conv_bwd_weight_acc).
 * seld_hcq_wgrad_supported: 1 if the shape is taken (algebra 4, 'same' stride-1 1x1 / 1x3 / 3x3, row length a multiple of
 * 32, Cout/4 a multiple of 16). */
int seld_hcq_wgrad_supported(const seld_conv_desc* desc, int32_t npair);
int seld_hcq_wgrad_label(const seld_conv_desc* desc, int32_t npair, char* buf, int32_t buflen);
int seld_hcq_wgrad_acc(const seld_conv_desc* desc, int32_t npair, const float* x, const float* dyA, const float* dyB,
                       float* const dwA[8], float* const dwB[8], void* stream);

/* SELD_DETERMINISTIC=1 (read with the other switches, seld_env_reload): reductions that are normally split over workgroups and
 * folded with float atomics -- BatchNorm statistics (seld_channel_stats), the two-pass BatchNorm / gate / pooling backward
 * reductions, linear-layer weight and bias gradients, the loss sum, the position splits of seld_hc_conv_bwd_weight* -- run as
 * ONE ordered chain per output element.  The host mirror then also keeps statistics out of the convolution epilogues and
 * takes the weight gradient below for every layer the grouped kernels do not take.
 * seld_hc_conv_bwd_weight_det: reproducible dw[c] += weight gradient of any convolution (real / quaternion / dual quaternion:
 * quaternion_ops.py:131-147, dual_quaternion_ops.py:122-153 differentiated), dbias += (nullable); workspace: Cout * Cin *
 * kh * kw floats.  Needs SELD_DETERMINISTIC set (SELD_EUNSUPPORTED otherwise). */
size_t seld_hc_conv_bwd_weight_det_workspace(const seld_conv_desc* desc);
int seld_hc_conv_bwd_weight_det(const seld_conv_desc* desc, const float* x, const float* dy, float* const dw[8], float* dbias,
                                void* workspace, size_t workspace_bytes, void* stream);

/* Weight gradients of a LIST of dual-quaternion convolutions in one grouped, persistent launch per shape family
 * (csrc/hcq_wgrad_grp.hip): dw[c] += d loss / d W_c for every job, i.e. dual_quaternion_conv
 * (dual_quaternion/dual_quaternion_ops.py:111-153) differentiated w.r.t. its eight component weights, which the reference
 * leaves to autograd through F.convNd (dual_quaternion_ops.py:153).  24 block products per layer; no atomics and a fixed
 * summation order: the result is reproducible from run to run.  x / dy: input and output-gradient tensors of the layer
 * (contiguous NCHW / NCT, desc.N images); dw: the eight component gradient tensors (Cout/8, Cin/8, kh, kw), accumulated into.
 * Shapes taken: algebra 8, 'same' stride-1 layers with rows of >= 128 positions (a multiple of 16) and
 * (Cout/8, Cin/8, kernel) = (48, 24, 1x3), (24, 48, 1x1), (24, 24, 3x3), (48, 48, 1x3): families 0..3, one persistent launch
 * per family present in the list.  seld_hcq_wgrad_group_workspace returns the scratch bytes (0: a job is not taken -- use the per-layer entry
 * points); the scratch needs no initialisation. */
typedef struct seld_wgrad_job {
    seld_conv_desc desc;
    const float* x;
    const float* dy;
    float* dw[8];
} seld_wgrad_job;
int seld_hcq_wgrad_group_family(const seld_conv_desc* desc);      /* 0..3 as listed above, -1 = not taken */
size_t seld_hcq_wgrad_group_workspace(const seld_wgrad_job* jobs, int32_t njobs);
int seld_hcq_wgrad_group(const seld_wgrad_job* jobs, int32_t njobs, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Elementwise / pooling / dropout   (torch.nn.ReLU/Tanh/MaxPool/Dropout at model.py:175-202,
 * 280-282, 449-451)
 * ------------------------------------------------------------------------------------------ */
int seld_act_fwd(const float* x, int64_t n, int32_t act, float* y, void* stream);
int seld_act_bwd(const float* dy, const float* y, int64_t n, int32_t act, float* dx, void* stream);

/* max pool over windows (ph, pw), stride = window, floor mode; x (NC, H, W) -> y (NC, H/ph, W/pw).
 * idx (uint8, nullable) receives the argmax position inside the window (row-major), as torch
 * keeps indices for backward. */
int seld_maxpool_fwd(const float* x, int64_t NC, int32_t H, int32_t W, int32_t ph, int32_t pw,
                     float* y, uint8_t* idx, void* stream);
int seld_maxpool_bwd(const float* dy, const uint8_t* idx, int64_t NC, int32_t H, int32_t W,
                     int32_t ph, int32_t pw, float* dx, void* stream);

/* dropout with a Philox-4x32-10 counter RNG: element i is kept iff u(seed, offset + i/4)[i%4] >= p.
 * `per_channel` (Dropout1d): one decision per (n, c) row of length S.  y = x * keep / (1 - p). */
/* `state` (nullable): device-resident step state (seld_step_begin below); state[0] is added to `offset`, so a launch
 * recorded in a HIP graph draws fresh numbers at every replay. */
int seld_dropout_fwd(const float* x, int64_t n, float p, uint64_t seed, uint64_t offset, const uint64_t* state,
                     float* y, void* stream);
int seld_dropout_mask_rows(int64_t rows, float p, uint64_t seed, uint64_t offset, const uint64_t* state,
                           float* mask, void* stream);

/* y = a + b ; y += b */
int seld_add(const float* a, const float* b, int64_t n, float* y, void* stream);
int seld_accumulate(float* dst, const float* src, int64_t n, void* stream);   /* dst += src */

/* ------------------------------------------------------------------------------------------
 * Multi-head self attention core (model.py:39-48): out = softmax(q k^T / sqrt(hd)) v, flash style
 * (the T x T energy tensor is never materialised).
 * q, k, v, out: (N, H*hd, T) -- the layout the 1x1 Conv1d projections of model.py:20-22 produce --
 * with head h on channels [h*hd, (h+1)*hd) (model.py:35-37).  hd <= 64.
 * lse (N, H, T): log-sum-exp of the scaled scores, saved for backward.
 * ------------------------------------------------------------------------------------------ */
int seld_mha_fwd(const float* q, const float* k, const float* v, int32_t N, int32_t T, int32_t H, int32_t hd,
                 float* out, float* lse, void* stream);
size_t seld_mha_bwd_workspace(int32_t N, int32_t T, int32_t H);
int seld_mha_bwd(const float* q, const float* k, const float* v, const float* out, const float* dout,
                 const float* lse, int32_t N, int32_t T, int32_t H, int32_t hd,
                 float* dq, float* dk, float* dv, void* workspace, size_t workspace_bytes, void* stream);
/* Self-attention on ONE projected tensor qkv (N, 3E, T) = [values | keys | queries] along the channels -- the three 1x1
 * projections of model.py:31-33 applied to the same input run as one convolution with the three weights stacked; dqkv has
 * the same layout, so one data-gradient and one weight-gradient launch follow.  Same arithmetic as seld_mha_fwd /
 * seld_mha_bwd on the three slices.  Matrix-core kernels only: SELD_EUNSUPPORTED unless seld_mha_packed_ok(T, hd) != 0
 * (hd in {16, 32, 48, 64}, T % 16 == 0).  workspace as seld_mha_bwd_workspace. */
int seld_mha_packed_ok(int32_t T, int32_t hd);
int seld_mha_fwd_packed(const float* qkv, int32_t N, int32_t T, int32_t H, int32_t hd, float* out, float* lse, void* stream);
int seld_mha_bwd_packed(const float* qkv, const float* out, const float* dout, const float* lse, int32_t N, int32_t T,
                        int32_t H, int32_t hd, float* dqkv, void* workspace, size_t workspace_bytes, void* stream);
/* Masked and cross-length attention (model.py:25-51 with a mask, or key_len != query_len):
 *   out = softmax(masked(q k^T) / sqrt(hd)) v, per head.
 * q, out, dq: (N, H*hd, Tq); k, v, dk, dv: (N, H*hd, Tk); lse (N, H, Tq): the saved row statistics.  hd <= 64.
 * keep (may be NULL: no mask): uint8 keep-mask over the (N, H, Tq, Tk) energy, element (n, h, q, k) at
 * keep[n*s[0] + h*s[1] + q*s[2] + k*s[3]] with s = mask_strides (elements, >= 0; 0 on a broadcast dim).  A score
 * whose keep byte is 0 is replaced by -1e9 / sqrt(hd) (masked_fill(mask == 0, -1e9) before the scaling): masked keys
 * of a partially masked row get weight exactly 0, and a fully masked row attends uniformly to all Tk keys (its output
 * is the mean of v; its lse is saved as +inf).  Backward follows masked_fill: a masked score has zero gradient, so a
 * fully masked row gives dq = 0, nothing to dk, and dout / Tk to every key's dv.
 * Dispatch: fp32 matrix cores for hd in {16, 32, 48, 64} with Tq % 16 == 0 and Tk % 16 == 0 (unless SELD_MHA_NO_MFMA),
 * the VALU kernels otherwise.  SELD_EINVAL (NULL tensor, a size <= 0, keep without strides or with a negative
 * stride), SELD_EUNSUPPORTED (hd > 64) and SELD_EWORKSPACE are returned before anything is written.  workspace:
 * seld_mha_bwd_ex_workspace(N, Tq, H) bytes. */
int seld_mha_fwd_ex(const float* q, const float* k, const float* v, int32_t N, int32_t Tq, int32_t Tk, int32_t H,
                    int32_t hd, const uint8_t* keep, const int64_t mask_strides[4], float* out, float* lse, void* stream);
size_t seld_mha_bwd_ex_workspace(int32_t N, int32_t Tq, int32_t H);
int seld_mha_bwd_ex(const float* q, const float* k, const float* v, const float* out, const float* dout,
                    const float* lse, int32_t N, int32_t Tq, int32_t Tk, int32_t H, int32_t hd, const uint8_t* keep,
                    const int64_t mask_strides[4], float* dq, float* dk, float* dv, void* workspace,
                    size_t workspace_bytes, void* stream);

/* (N, C, T) <-> (N, T, C) transposes (the permutes of model.py:30-37, 220-222, 318) */
int seld_transpose_nct_ntc(const float* x, int32_t N, int32_t C, int32_t T, float* y, void* stream);
int seld_transpose_ntc_nct(const float* x, int32_t N, int32_t T, int32_t C, float* y, void* stream);

/* ------------------------------------------------------------------------------------------
 * Loss (train.py:186-204): loss = w_sed * BCELoss(sed, t_sed) + w_doa * MSELoss(doa, t_doa), mean
 * reductions (train.py:498-499); sed/doa are the model OUTPUTS (after Sigmoid / Tanh).
 * target is (rows, n_sed + n_doa) row-major as produced by the preprocessing (train.py:191-192).
 * WRITES the scalar to loss[0] (workgroup sums added in a fixed order by the last workgroup to finish: no pre-zeroing,
 * run-to-run identical; the scratch is a per-device static of the library, so evaluations on ONE device must not overlap
 * on different streams) and, if non-null, writes dloss/dsed and dloss/ddoa (torch.nn.BCELoss semantics: logs clamped at
 * -100, backward denominator >= 1e-12).
 * ------------------------------------------------------------------------------------------ */
int seld_loss_fwd_bwd(const float* sed, const float* doa, const float* target,
                      int64_t rows, int32_t n_sed, int32_t n_doa, float w_sed, float w_doa,
                      float* loss, float* dsed, float* ddoa, void* stream);

/* The same loss, permutation invariant over the `overlaps` (1..3) same-class track slots.  Layouts: sed[r, c * O + o],
 * doa[r, (c * O + o) * 3 + d], target[r] = [t_sed (C * O) | t_doa (3 * C * O)].  With a = w_sed / (rows * C * O) and
 * b = w_doa / (rows * 3 * C * O), the pair cost of prediction slot o against target slot j of a cell (r, c) is
 *     P[o][j] = a * bce(sed[o], t_sed[j]) + b * sum_d (doa[o][d] - t_doa[j][d])^2        (logs clamped at -100)
 * and a permutation pi (prediction slot -> target slot) costs (P[0][pi0] + P[1][pi1]) + P[2][pi2] (the terms of
 * missing slots absent).  Permutations are numbered in lexicographic order -- O = 3: 0 (0,1,2), 1 (0,2,1), 2 (1,0,2),
 * 3 (1,2,0), 4 (2,0,1), 5 (2,1,0); O = 2: 0 (0,1), 1 (1,0) -- and the search starts from the identity and moves on `<`
 * only: ties go to the lowest index, a NaN cost never displaces the identity.  loss[0] is WRITTEN with the sum over
 * cells of the chosen cost; dsed / ddoa (nullable, as above) are the plain loss's gradients with each cell's target
 * slots permuted by the chosen pi (the choice is a constant; DOA terms are not masked by activity).
 * perm (nullable): (rows, classes) int32, the chosen index.  parts (nullable): 2 floats, the a * BCE and b * MSE sums of
 * the chosen pairing.  One launch.  It shares the per-device reduction scratch of seld_loss_fwd_bwd: evaluations of
 * EITHER loss on one device must not overlap on different streams.
 * SELD_EINVAL: NULL sed / doa / target / loss or a size <= 0; SELD_EUNSUPPORTED: overlaps > 3. */
int seld_loss_pit_fwd_bwd(const float* sed, const float* doa, const float* target,
                          int64_t rows, int32_t classes, int32_t overlaps, float w_sed, float w_doa,
                          float* loss, float* dsed, float* ddoa, int32_t* perm, float* parts, void* stream);

/* ------------------------------------------------------------------------------------------
 * Adam (torch.optim.Adam defaults, train.py:502) over ONE flat fp32 buffer that holds every
 * parameter; grads/exp_avg/exp_avg_sq are parallel flat buffers.  step is 1-based.
 * The gradient used is g' = fma(weight_decay, param, grad * grad_scale): coupled (L2) weight decay, one rounding.
 * ------------------------------------------------------------------------------------------ */
int seld_adam_flat(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                   float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step,
                   float grad_scale, void* stream);

/* Device-resident step state, so that one training step (train.py:552-560) can be recorded once as a HIP graph and
 * replayed: 4 x uint64 = { Philox base added to every dropout offset, optimiser step (1-based), learning rate (float
 * bits in the low word), Philox draws per step }.
 * seld_step_begin replaces `optimizer.zero_grad()` (train.py:552): zeroes the flat gradient buffer (n floats, 16-byte
 * aligned) and, if state is non-null, advances state[1] += 1.
 * seld_adam_flat_state is seld_adam_flat with step = state[1] and lr = state[2]; as the last launch of a step it also
 * moves the Philox base past the step's draws, state[0] += state[3].
 * Both calls update the state for n == 0 as well (a step over no parameters is still a step: state[1] advances at its
 * start and state[0] at its end); seld_adam_flat_state used to return early there and left the Philox base behind. */
int seld_step_begin(float* flat_grad, int64_t n, uint64_t* state, void* stream);
int seld_adam_flat_state(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                         float beta1, float beta2, float eps, float weight_decay, float grad_scale,
                         uint64_t* state, void* stream);

/* ------------------------------------------------------------------------------------------
 * The optimiser's extras: clipping by global norm, decoupled (AdamW) decay, an exponential moving average of the weights.
 *
 * seld_grad_norm: one launch, nothing read back, no float atomics.  With x[i] = grad[i] * grad_scale rounded to fp32 (the
 * product seld_adam_flat forms), squares and sums in fp64 and ONE rounding to fp32 after the square root, it writes
 *     clip[0] = ||x||_2
 *     clip[1] = min(1, max_norm / (clip[0] + 1e-6f))      torch.nn.utils.clip_grad_norm_'s coefficient: an infinite norm
 *                                                         gives 0, a NaN norm NaN; no step is skipped
 *     clip[2] = max(clip[2], clip[0])                     the largest norm since the host zeroed it (a NaN norm is not kept)
 *     clip[3] += (clip[1] < 1)                            the steps that were clipped since the host zeroed it
 * clip: 4 floats on the device.  The grid depends on n alone and the workgroup sums are added in a fixed order by the last
 * workgroup to finish, so two runs give the same bits; the scratch is a per-device static of the library (not the loss
 * kernels'), so launches on ONE device must not overlap on different streams.  n == 0: norm 0, coefficient 1.
 * SELD_EINVAL: NULL grad with n > 0, NULL clip, n < 0, max_norm not greater than 0.
 *
 * seld_adam_flat_ex / seld_adam_flat_state_ex: seld_adam_flat / seld_adam_flat_state with, per element,
 *     g' = (grad * grad_scale) * clip[1]                  clip (nullable) read on the device; NULL: no multiply
 *     decoupled == 0:  g' = fma(weight_decay, p, g')      as seld_adam_flat
 *     decoupled != 0:  p <- p * (1 - lr * weight_decay)   torch.optim.AdamW; g' gets no decay term
 *     m, v and the update as seld_adam_flat
 *     ema = d * ema + (1 - d) * p_new,  d = min(ema_decay, (1 + step) / (10 + step))      ema nullable; step 1-based
 *         (evaluated as ema + (1 - d) * (p_new - ema): an average equal to the weight stays on it bit for bit)
 * With clip NULL, ema NULL and decoupled 0 they give the bits of seld_adam_flat / seld_adam_flat_state.  The state entry
 * ends the step as seld_adam_flat_state does (state[0] += state[3]), for n == 0 too.
 * SELD_EINVAL: as seld_adam_flat / seld_adam_flat_state, or ema given with an ema_decay outside [0, 1).
 * ------------------------------------------------------------------------------------------ */
int seld_grad_norm(const float* grad, int64_t n, float grad_scale, float max_norm, float* clip, void* stream);
int seld_adam_flat_ex(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                      float lr, float beta1, float beta2, float eps, float weight_decay, int32_t decoupled,
                      int32_t step, float grad_scale, const float* clip, float ema_decay, void* stream);
int seld_adam_flat_state_ex(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                            float beta1, float beta2, float eps, float weight_decay, int32_t decoupled,
                            float grad_scale, const float* clip, float ema_decay, uint64_t* state, void* stream);

/* ------------------------------------------------------------------------------------------
 * STFT magnitude / phase (utility_functions.py:129-155 = scipy.signal.stft(window='hamming',
 * boundary='zeros', padded=True) -> abs/angle -> drop DC bin -> drop last frame).
 * x (C, L) fp32; out (C or 2C, nperseg/2, frames-1) fp32, phase channels after magnitude channels.
 * nperseg: any length 2 <= nperseg <= 4096 (the reference uses 512); longer segments return SELD_EUNSUPPORTED.
 * Lengths that are not 7-smooth (2^a 3^b 5^c 7^d) run as a Bluestein transform and need a workspace of
 * seld_stft_workspace(nperseg) bytes: only seld_stft_magphase_ws serves them, the two calls without a workspace
 * return SELD_EWORKSPACE there.
 * ------------------------------------------------------------------------------------------ */
int seld_stft_frames(int32_t L, int32_t nperseg, int32_t noverlap);   /* frames AFTER the cut */
int seld_stft_magphase(const float* x, int32_t C, int32_t L, int32_t nperseg, int32_t noverlap,
                       int32_t output_phase, float* out, void* stream);
/* The same with every argument of spectrum_fast (utility_functions.py:129-130): cut_dc = 0 keeps all nperseg/2 + 1
 * bins, cut_last_timeframe = 0 keeps the last frame; `window` (nullable, device, nperseg floats) = window values
 * already divided by their sum (scipy's scaling='spectrum'), null = periodic Hamming (window='hamming').
 * out (C or 2C, nperseg/2 + 1 - cut_dc, seld_stft_frames_ex(...)). */
int seld_stft_frames_ex(int32_t L, int32_t nperseg, int32_t noverlap, int32_t cut_last_timeframe);
int seld_stft_magphase_ex(const float* x, int32_t C, int32_t L, int32_t nperseg, int32_t noverlap,
                          int32_t output_phase, int32_t cut_dc, int32_t cut_last_timeframe,
                          const float* window, float* out, void* stream);
/* Bytes of device workspace seld_stft_magphase_ws needs for a segment length (0: none; the power-of-two lengths
 * <= 1024 and every 7-smooth length need none).  The workspace is rewritten by every call (the chirp and its
 * spectrum), so one buffer may serve calls on one stream in turn. */
size_t seld_stft_workspace(int32_t nperseg);
/* seld_stft_magphase_ex with a caller-provided workspace of at least seld_stft_workspace(nperseg) bytes
 * (SELD_EWORKSPACE, nothing launched, if it is smaller).  Serves every length 2 <= nperseg <= 4096. */
int seld_stft_magphase_ws(const float* x, int32_t C, int32_t L, int32_t nperseg, int32_t noverlap,
                          int32_t output_phase, int32_t cut_dc, int32_t cut_last_timeframe,
                          const float* window, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* seld_stft_magphase_ws, but out (2C, bins, frames): plane c = Re Z of channel c, plane C + c = Im Z (same scaling:
 * the window divided by its sum).  Same refusals, nothing launched on refusal. */
int seld_stft_complex_ws(const float* x, int32_t C, int32_t L, int32_t nperseg, int32_t noverlap,
                         int32_t cut_dc, int32_t cut_last_timeframe, const float* window, float* out,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Log-power and first-order-Ambisonics intensity-vector features of complex spectra, linear in
 * frequency or projected onto bands (a mel filterbank); csrc/spatial_features.hip.
 * z (2C, bins, frames) as seld_stft_complex_ws writes it.
 * kind:   0 LOGPOWER     out (C, bands, frames)          log(P + eps) per channel
 *         1 IV           out (3C/4, bands, frames)       per group of 4 channels [W, D1, D2, D3]: three components
 *         2 LOGPOWER_IV  layout 0: out (C + 3C/4, ...)   all log-power planes, then the IV planes of group 0, 1, ...
 *                        layout 1: out (C, ...)          per group [log-power of W, I1, I2, I3] (one quaternion)
 * Per bin k: p_c = |Z_c|^2;  E = eps + |W|^2 + (|D1|^2 + |D2|^2 + |D3|^2) / 3;  i_d = Re(conj(W) D_d) / E.
 * fb == NULL: bands == bins, P = p, I_d = i_d.
 * fb (bands, bins) fp32, band_lo / band_hi (bands) int32 = first and one-past-last bin of each band that may be
 *   nonzero:  P[m] = sum_k fb[m,k] p[k],  I_d[m] = sum_k fb[m,k] i_d[k]  (normalised per bin, then projected: the
 *   DCASE baseline's order), sums over band_lo[m] <= k < band_hi[m], clamped to [0, bins) by the kernel, taken in
 *   the order of k.  No atomics: results are run-to-run identical.
 * SELD_EINVAL, before any HIP call: z or out NULL; C, bins, frames or bands < 1; an unknown kind or layout; an IV kind
 *   with C % 4 != 0; layout 1 with kind != 2; eps <= 0 or NaN; fb without band_lo / band_hi; fb == NULL with
 *   bands != bins.  SELD_EUNSUPPORTED: a plane of z or out of 2^31 floats or more, more than 65535 channels (kind 0)
 *   or groups.  A refused call launches nothing and writes nothing.
 * ------------------------------------------------------------------------------------------ */
#define SELD_FEAT_LOGPOWER     0
#define SELD_FEAT_IV           1
#define SELD_FEAT_LOGPOWER_IV  2
#define SELD_FEAT_LAYOUT_GROUPED     0
#define SELD_FEAT_LAYOUT_QUATERNION  1
int seld_spatial_features_channels(int32_t C, int32_t kind, int32_t layout);      /* planes of out, or SELD_EINVAL */
int seld_spatial_features(const float* z, int32_t C, int32_t bins, int32_t frames, int32_t kind, int32_t layout,
                          const float* fb, const int32_t* band_lo, const int32_t* band_hi, int32_t bands,
                          float eps, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Dataset normalisation, in place on a resident predictor array x (items, channels, hw) fp32
 * (SURVEY 8(f) N1).
 * seld_dq_unit_norm replaces train.py:257-275 (and its copies for the validation / test arrays,
 *   277-308): channels 0..7 of every position are one dual quaternion (q, p); p <- p - (q.p/|q|^2) q,
 *   q <- q/|q|.  channels >= 8; further channels are left untouched.  Same operation order as the
 *   reference's torch expressions, every operation correctly rounded (a zero q yields NaN there and here).
 * seld_group_standardize replaces train.py:341-349 (and 350-405 for the other arrays / groups):
 *   g = x[:, c0:c1]; g <- (g - mean(g)) / std(g) with one scalar mean and one population std over the
 *   whole group.  work: 3 doubles of device scratch (cleared by the call); mean_std: 2 device floats
 *   receiving the float32 mean and std that were applied, or NULL.  An empty group is SELD_EINVAL.
 * ------------------------------------------------------------------------------------------ */
int seld_dq_unit_norm(float* x, int64_t items, int32_t channels, int64_t hw, void* stream);
int seld_group_standardize(float* x, int64_t items, int32_t channels, int32_t c0, int32_t c1, int64_t hw,
                           double* work, float* mean_std, void* stream);

/* ------------------------------------------------------------------------------------------
 * Post-processing + test metrics of evaluate_test (train.py:84-130) for a batch of
 * recordings whose outputs are resident: sed (clips, frames, classes*overlaps), doa (clips, frames,
 * 3*classes*overlaps), target (clips, frames, 4*classes*overlaps) = [activity | location] as the
 * reference's joint target.  One call replaces, per recording, gen_submission_list_task2
 * (utility_functions.py:184-210) on prediction and target, location_sensitive_detection
 * (metrics.py:123-182), segment_labels (Dcase21_metrics.py:239-278) and
 * SELDMetrics.update_seld_scores (Dcase21_metrics.py:51-154), and ADDS to
 *   counters[13] = { TP, FP, FN (L3DAS21, summed as train.py:124-126) ;
 *                    _TP, _FP, _FN, _S, _D, _I, _Nref, _DE_TP, _DE_FP, _DE_FN of SELDMetrics }
 *   total_de[1]  = SELDMetrics._total_DE
 * (device memory, zeroed by the caller before the first recording).  The scores of train.py:131-150 /
 * compute_seld_scores are a dozen scalar operations on these and stay on the host.
 * frames > num_frames is SELD_EINVAL; overlaps > 3, classes*overlaps > 64 or frames_per_block > 64 are
 * SELD_EUNSUPPORTED (the reference uses 14 x 3 and 10).
 * ------------------------------------------------------------------------------------------ */
#define SELD_METRIC_COUNTERS 13
int seld_metrics_accumulate(const float* sed, const float* doa, const float* target, int32_t clips, int32_t frames,
                            int32_t num_frames, int32_t classes, int32_t overlaps, float max_loc_value,
                            double spatial_threshold, double doa_threshold, int32_t frames_per_block,
                            int64_t* counters, double* total_de, void* stream);

/* ------------------------------------------------------------------------------------------
 * Scoring event lists (csrc/event_metrics.hip): the same counters from rows instead of dense outputs.
 * Replaces location_sensitive_detection and sed_score_computation (metrics.py:123-288) and segment_labels +
 * SELDMetrics.update_seld_scores (Dcase21_metrics.py:239-278, 51-154) for a batch of recordings:
 *   pred_rows (pred_count, 5), true_rows (true_count, 5)   double { frame, class, x, y, z }, recording-major:
 *                                                          the `rows` of seld_decode_write
 *   pred_offsets, true_offsets (recordings + 1)            int64, its `rec_offsets`
 * Inside a recording the rows are sorted by frame (ascending; the caller sorts, stably: the order of the rows of
 * one frame is the order of the reference's lists, and the position of an event among its frame's events of its
 * class is its track).  Offsets are forced into [0, count] and into ascending order before use, so no row
 * outside the lists is read whatever they hold.  ADDS to
 *   counters[16] = the 13 of seld_metrics_accumulate, in that order, then TP, FP, FN of sed_score_computation
 *   total_de[1]  = SELDMetrics._total_DE
 * and WRITES
 *   flags[0] = rows (both lists) whose frame is not an integer in [0, n_frames): the reference's KeyError.  They
 *              take no part in counters[0..2] and [13..15].
 *   flags[1] = (recording, frame, class) cells of either list with more than 3 events, among integer classes
 *              below nb_classes and integer frames of a block.  The association is solved for 3 x 3 at most:
 *              when flags[1] is not zero the call is REFUSED and adds nothing to counters and total_de.
 * Location-sensitive detection has no limit on the events of a frame.  The block metrics run over
 * ceil(n_frames / frames_per_block) blocks; a block covers its frames_per_block frames also beyond n_frames, as
 * segment_labels does; classes that are no integer in [0, nb_classes) are ignored there.  nb_classes = 0 leaves
 * the block metrics out altogether (counters[3..12] and total_de untouched, flags[1] = 0).
 * Cartesian coordinates only.  SELD_EINVAL: nb_classes outside [0, 64], frames_per_block < 1, a negative count,
 * n_frames < 0, a NULL pointer that is needed.  SELD_EUNSUPPORTED: a list of 2^28 rows or more (nothing is launched).
 * A row with a NaN frame belongs to no block and is counted in flags[0] only; torch.sort puts such rows last.  Two launches and one 16-byte memset, no workspace, no host read:
 * the call can be recorded in a graph.
 * ------------------------------------------------------------------------------------------ */
#define SELD_EVENT_METRIC_COUNTERS 16
#define SELD_EVENT_METRICS_MAX_TRACKS 3
int seld_event_metrics_accumulate(const double* pred_rows, const int64_t* pred_offsets, int64_t pred_count,
                                  const double* true_rows, const int64_t* true_offsets, int64_t true_count,
                                  int64_t recordings, int32_t n_frames, int32_t nb_classes, int32_t frames_per_block,
                                  double spatial_threshold, double doa_threshold, int64_t* counters, double* total_de,
                                  int64_t* flags, void* stream);

/* ------------------------------------------------------------------------------------------
 * seld_event_metrics_accumulate_ex: the call above with two more arguments behind frames_per_block.
 *   coords      3: rows are (count, 5) double { frame, class, x, y, z }, as above.
 *               2: rows are (count, 4) double { frame, class, azimuth, elevation } in DEGREES, as DCASE label
 *                  files give them.  The distance is the reference's for two-entry DOAs, operation by operation
 *                  with contraction off: v * pi / 180. first, then sin(e1) sin(e2) + cos(e1) cos(e2) cos(|a1 - a2|),
 *                  clipped to [-1, 1], acos(..) * 180 / pi (distance_between_spherical_coordinates_rad).
 *                  counters[0..2] are Euclidean and have no meaning for such rows: NOTHING is added to them;
 *                  counters[3..12] and [13..15] are computed; nb_classes = 0 adds to [13..15] alone.
 *   max_tracks  1 .. 8: events of one (recording, frame, class) cell the association takes; flags[1] counts
 *               the cells with more, and a call with flags[1] != 0 is refused and adds nothing, as above.
 * A cell of g references and q predictions costs a minimum-cost matching of min(g, q) pairs
 * (scipy.optimize.linear_sum_assignment).  Where several matchings cost the same, the first row -> column map in
 * lexicographic order wins, an unmatched row counting as a column above every real one.  Cells with at most 3
 * events on both sides are solved by the same code under every max_tracks, so they give the same bits.
 * SELD_EINVAL: coords outside {2, 3}, max_tracks outside [1, 8], and everything that is SELD_EINVAL above.
 * seld_event_metrics_accumulate(...) is this call with coords = 3 and max_tracks = 3.
 *
 * seld_least_distance: least_distance_between_gt_pred (Dcase21_metrics.py:191-220) for a batch.  Problem b has
 * gt_counts[b] reference and pred_counts[b] predicted DOAs of `coords` doubles each, the first entries of
 * gt[b] and pred[b] in padded (problems, 8, coords) arrays: Cartesian { x, y, z } as they are, spherical
 * { azimuth, elevation } in RADIANS, as the reference's function takes them.  Counts are forced into [0, 8] on the
 * device (the caller refuses longer lists).  WRITES, per problem, n = min(g, q) pairs:
 *   cost (problems, 8) double, row, col (problems, 8) int32: pair k < n is reference row[k] with prediction
 *        col[k] at cost[k] degrees, rows ascending as scipy returns them; entries from n on are 0 / -1 / -1
 *   pairs (problems) int32 = n
 * by the device functions of the scoring kernel (same distances, same tie rule).  SELD_EINVAL: problems < 0,
 * coords outside {2, 3}, a NULL pointer with problems > 0; SELD_EUNSUPPORTED: 2^28 problems or more.  One launch,
 * no workspace, no host read.
 * ------------------------------------------------------------------------------------------ */
#define SELD_EVENT_METRICS_MAX_TRACKS_EX 8
int seld_event_metrics_accumulate_ex(const double* pred_rows, const int64_t* pred_offsets, int64_t pred_count,
                                     const double* true_rows, const int64_t* true_offsets, int64_t true_count,
                                     int64_t recordings, int32_t n_frames, int32_t nb_classes, int32_t frames_per_block,
                                     int32_t coords, int32_t max_tracks, double spatial_threshold, double doa_threshold,
                                     int64_t* counters, double* total_de, int64_t* flags, void* stream);
int seld_least_distance(const double* gt, const int32_t* gt_counts, const double* pred, const int32_t* pred_counts,
                        int64_t problems, int32_t coords, double* cost, int32_t* row, int32_t* col, int32_t* pairs,
                        void* stream);

/* ------------------------------------------------------------------------------------------
 * The same counters broken down by recording and class.  For R recordings and C = nb_classes
 * (0 .. 64) both calls below WRITE (not add to; nothing needs zeroing) the tables
 *   counters (R, C + 2, 16) int64    in the order of seld_event_metrics_accumulate's counters
 *   total_de (R, C + 2)     double
 * Row c < C of a recording is what class c contributes; row C ("other") takes the list rows whose class is no integer
 * in [0, C): they take part in counters 0..2 and 13..15 alone, so counters 3..12 and total_de of that row are 0;
 * row C + 1 ("all") is what the plain call adds for this recording alone.
 *   counters 3, 4, 5, 9..12, total_de   what the class adds in each block (row "all": the sum over the classes)
 *   counters 6, 7, 8 (S, D, I)          class rows: min(fp, fn), max(0, fn - fp), max(0, fp - fn) of the class's own
 *                                       loc_FP / loc_FN in each block (the class-wise definition of DCASE's macro
 *                                       average); row "all": the reference's, loc_FP / loc_FN summed over the classes
 *                                       of the block first.  The only counters whose row "all" is not the sum of rows 0..C.
 *   counters 0..2 and 13..15            row by row: a prediction adds 1 to the FP of its class (2 where its frame has
 *                                       no reference row at all); a reference adds 2 to the FN of its class where its
 *                                       frame has no prediction row at all, else TP + 1 and FP - 1 when matched (by a
 *                                       prediction of its class), FN + 1 when not.  A class's FP can be negative.
 * Every (recording, block) unit writes a slab of (C + 2) x 17 eight-byte words into `workspace`, and a second kernel
 * adds the slabs of a recording in ascending block order: no atomics on memory, integer entries exact, total_de
 * entries the same bits every run.  The matching is the code of the plain calls, so the tables cannot disagree with
 * the totals about a match.
 *   seld_metrics_breakdown_workspace   bytes of workspace: recordings * ceil(n_frames / frames_per_block) * (C + 2) *
 *                                      17 * 8 (0 for arguments the calls refuse).  For the dense call, recordings =
 *                                      clips, n_frames = frames, nb_classes = classes.
 *   seld_event_metrics_breakdown       the arguments, flags, refusals and error codes of
 *                                      seld_event_metrics_accumulate_ex; coords = 2 leaves counters 0..2 zero; a call
 *                                      refused for an overflowing cell (flags[1] != 0) writes both tables as zeros.
 *   seld_metrics_breakdown             the arguments and error codes of seld_metrics_accumulate (clips are the
 *                                      recordings); counters 13..15 and row "other" stay zero.  SELD_EUNSUPPORTED also
 *                                      where the slab no longer fits the workgroup's LDS beside the wave's slice.
 * SELD_EWORKSPACE: workspace NULL or smaller than the query's answer; nothing is launched.  No host read: the calls
 * can be recorded in a graph (the workspace then belongs to the graph).
 * ------------------------------------------------------------------------------------------ */
size_t seld_metrics_breakdown_workspace(int64_t recordings, int32_t n_frames, int32_t nb_classes, int32_t frames_per_block);
int seld_event_metrics_breakdown(const double* pred_rows, const int64_t* pred_offsets, int64_t pred_count,
                                 const double* true_rows, const int64_t* true_offsets, int64_t true_count,
                                 int64_t recordings, int32_t n_frames, int32_t nb_classes, int32_t frames_per_block,
                                 int32_t coords, int32_t max_tracks, double spatial_threshold, double doa_threshold,
                                 int64_t* counters, double* total_de, void* workspace, size_t workspace_bytes,
                                 int64_t* flags, void* stream);
int seld_metrics_breakdown(const float* sed, const float* doa, const float* target, int32_t clips, int32_t frames,
                           int32_t num_frames, int32_t classes, int32_t overlaps, float max_loc_value,
                           double spatial_threshold, double doa_threshold, int32_t frames_per_block,
                           int64_t* counters, double* total_de, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Event decoding: the submission rows of resident network outputs (csrc/decode.hip).  Replaces
 * gen_submission_list_task2_OLD (utility_functions.py:158-181) and gen_submission_list_task2
 * (utility_functions.py:184-210), which train.py:110-116 calls on the prediction and on the target of
 * every test recording, for a batch: sed (recordings, frames, n), doa (recordings, frames, 3n),
 * n = classes * overlaps, both contiguous float32 (SELD_DECODE_F32) or both float64 (SELD_DECODE_F64).
 * Slot j of a frame is class j / overlaps, event j % overlaps, coordinates doa[.., 3j : 3j + 3].  A slot
 * is active when rint(sed) != 0 (half to even: 0.5 is off, 1.5 and -0.6 are on) and the frame's rounded
 * activities do not sum to zero; that sum is exact in any order for |sed| < 2^18 and nothing is promised
 * beyond.  Rows come out recording-major, frame-major, slot order:
 *   rows[e]  = { frame, class, x, y, z } as doubles; float32 input: x = (double)(doa * (float)max_loc_value),
 *              one float32 multiply then widened; float64 input: the multiply is in double
 *   event[e] = j % overlaps (the fifth entry of the reference's per-frame dict)
 *   rec_offsets[r] .. rec_offsets[r + 1] = the rows of recording r (recordings + 1 entries, CSR style)
 * The row count depends on the data, so the work is two calls on one stream:
 *   seld_decode_workspace  bytes of workspace both calls need (0 for a refused shape)
 *   seld_decode_count      reads sed once; leaves the total row count E as an int64 in the first 8 bytes
 *                          of the workspace (one device-to-host copy) and the frames' masks behind it
 *   seld_decode_write      takes the SAME workspace, untouched since the count call on the same shape, and
 *                          caller-allocated rows (capacity, 5), event (capacity), rec_offsets
 *                          (recordings + 1); capacity >= E; rows beyond capacity are not written; rows and
 *                          event may be NULL when capacity is 0.  Reads doa for active slots only.
 * No atomics: two runs give the same bytes.  Non-positive sizes, an unknown dtype, a negative capacity
 * and NULL pointers are SELD_EINVAL; classes * overlaps > 64 (one wave's ballot) or recordings * frames >=
 * 2^31 are SELD_EUNSUPPORTED (overlaps itself is not limited: decoding has no association step); a missing
 * or short workspace is SELD_EWORKSPACE.  A refused call launches nothing and writes nothing.
 * The offsets are scanned by ONE workgroup in dependent tiles of 1024 chunks of 64 frames: 5 tiles for 500 x 600
 * frames, 32768 serial tiles at the 2^31 - 1 frame limit, which is accepted but not what the scan is sized for.
 * ------------------------------------------------------------------------------------------ */
#define SELD_DECODE_F32 0
#define SELD_DECODE_F64 1
size_t seld_decode_workspace(int64_t recordings, int32_t frames, int32_t classes, int32_t overlaps);
int seld_decode_count(const void* sed, int32_t dtype, int64_t recordings, int32_t frames, int32_t classes,
                      int32_t overlaps, void* workspace, size_t workspace_bytes, void* stream);
int seld_decode_write(const void* doa, int32_t dtype, int64_t recordings, int32_t frames, int32_t classes,
                      int32_t overlaps, double max_loc_value, const void* workspace, size_t workspace_bytes,
                      double* rows, int32_t* event, int64_t capacity, int64_t* rec_offsets, void* stream);

/* ------------------------------------------------------------------------------------------
 * Target encoding and segmentation: the preparation half's label path (csrc/labels.hip).
 *
 * seld_encode_events replaces the fill loop of csv_to_matrix_task2 (utility_functions.py:219-267) for a batch of
 * recordings, and is the exact inverse of the decode kernel above.  Events are CSR by recording, all on the device:
 *   first_frame[E], last_frame[E]   int32, inclusive; last < first covers no frame (np.arange is empty)
 *   cls[E]                          int32 class id
 *   xyz[E, 3]                       double
 *   rec_offsets[R + 1]              int64: events rec_offsets[r] .. rec_offsets[r + 1] belong to recording r
 *   events = E; max_rec_events      the largest event count of one recording, as the caller knows it from the offsets
 *                                   it built (it sizes the LDS staging); a recording that holds more is counted invalid
 * target (R, frames, 4 * classes * overlaps), or (R, frames, 4 * classes) with no_overlaps != 0, contiguous, float32
 * (SELD_DECODE_F32) or float64 (SELD_DECODE_F64); per frame [cl (classes * slots) | loc (classes * slots * 3)], slot
 * class * slots + pos, as the reference stacks it.
 *   * an event takes, in every frame it covers, the next free slot of its class IN EVENT ORDER within the recording
 *     (the reference's pos = int(np.sum(cl[f][class_id])));
 *   * loc = xyz / max_loc_value, divided in double; float32 output is that quotient rounded once; an empty loc slot is
 *     0.0 / max_loc_value, as the reference divides the whole array;
 *   * every element of target is written exactly once, zeros included: the caller does not clear it;
 *   * overflow[0] receives the number of (recording, frame, class) cells that more than `overlaps` events want (the
 *     reference raises IndexError there; with no_overlaps only slot 0 is emitted but the cells are still counted, as
 *     the reference fills before it slices), overflow[1] the number of invalid events and recordings: a covered frame
 *     outside [0, frames), a class outside [0, classes), offsets that are not ascending inside [0, E], more than
 *     max_rec_events events.  Invalid events are skipped; nothing is ever written outside target.  The two ints are
 *     cleared by the call (a memset node on the stream) and are the only words touched by atomics: target has one
 *     writer per element, two runs give the same bytes.
 * SELD_EINVAL: a NULL pointer (the four event arrays may be NULL when events == 0), non-positive recordings / frames /
 * classes / overlaps, events < 0, max_rec_events outside [0, events], an unknown dtype.  SELD_EUNSUPPORTED:
 * classes * overlaps > 64, max_rec_events > SELD_ENCODE_MAX_EVENTS, 2^31 workgroups or more.  A refused call launches
 * nothing and writes nothing.
 *
 * seld_segment cuts overlapping, zero-padded segments (segment_task2, utility_functions.py:302-342, and
 * segment_waveforms, :272-299):
 *   layout SELD_SEGMENT_TIME_LAST    src (rows, length)  -> dst (segments, rows, seg_len)
 *                                    dst[s, r, j] = src[r, s * hop + j], or 0 when s * hop + j >= length
 *   layout SELD_SEGMENT_TIME_FIRST   src (length, rows)  -> dst (segments, seg_len, rows)
 *                                    dst[s, j, r] = src[s * hop + j, r], or 0 when s * hop + j >= length
 * float32 or float64 (dtype as above), hop >= 1, `segments` as the caller wants them.  16-byte loads and stores where
 * the pointers and the extents allow, scalar loads at ragged edges and for odd hops, a scalar kernel otherwise.
 * SELD_EINVAL: a NULL pointer, a non-positive extent, hop < 1, an unknown dtype or layout; SELD_EUNSUPPORTED: rows *
 * length, rows * seg_len or segments * hop of 2^46 or more.  A refused call launches nothing.
 * ------------------------------------------------------------------------------------------ */
#define SELD_ENCODE_MAX_EVENTS 4096
#define SELD_SEGMENT_TIME_LAST  0
#define SELD_SEGMENT_TIME_FIRST 1
int seld_encode_events(const int32_t* first_frame, const int32_t* last_frame, const int32_t* cls, const double* xyz,
                       const int64_t* rec_offsets, int64_t events, int32_t max_rec_events, int64_t recordings,
                       int32_t frames, int32_t classes, int32_t overlaps, double max_loc_value, int32_t no_overlaps,
                       int32_t dtype, void* target, int32_t* overflow, void* stream);
int seld_segment(const void* src, int32_t dtype, int32_t layout, int64_t rows, int64_t length, int64_t seg_len,
                 int64_t hop, int64_t segments, void* dst, void* stream);

/* ------------------------------------------------------------------------------------------
 * Device-resident epoch loader (csrc/loader.hip): what a training step needs from a DataLoader over resident arrays,
 * as two launches that can be recorded in a HIP graph.  None of the entry points allocates or synchronises.
 *
 * seld_gather_rows fetches one minibatch.  For b in [0, count):
 *     p = (cursor ? cursor[0] * cursor_stride : 0) + start + b
 *     out_x[b, :] = x_all[index[p], :]        out_y[b, :] = y_all[index[p], :]
 *   x_all (n_rows, row_x), y_all (n_rows, row_y), out_x (B, row_x), out_y (B, row_y): contiguous fp32; index: n_index
 *   int64 on the device; cursor: ONE int32 on the device that the kernel reads, so a recorded launch fetches another
 *   batch at every replay with no host write in between (NULL: only `start` selects).  Either the x or the y pair may be
 *   NULL (both pointers of the pair).  Output rows [count, B) are not touched.
 *   A position p outside [0, n_index) or an index[p] outside [0, n_rows) reads nothing and ZERO-FILLS its output
 *   rows: a defined, fault-free result (a cursor that ran past the epoch yields zero batches).
 *   16-byte loads and stores where a row's source and destination are 16-byte aligned together, single floats before
 *   and behind that part, and for a row whose two sides are aligned differently.
 *   SELD_EINVAL: index NULL, neither pair given, half a pair, a non-positive n_index / n_rows / row length / B / count,
 *   count > B, count > 65535, a negative cursor_stride.  Nothing is launched on refusal.
 * seld_gather_rows_aug is seld_gather_rows with a per-sample augmentation applied on the way: a signed permutation of
 * the predictor channels together with the matching transform of the DOA labels, and frequency / time masks.  Same
 * addressing, same bytes moved, one launch, recordable.  A position or index out of range ZERO-FILLS its rows and
 * nothing else is applied to them; output rows [count, B) are not touched.
 *   Geometry: a predictor row is (C, F, T), row_x = C * F * T, C <= 16; a target row is (T_out, y_cols) with
 *   y_cols = 4 * n_sed = [n_sed activity | n_sed * 3 location], the location of slot s and axis a at column
 *   n_sed + 3 * s + a (what seld_encode_events writes); row_y is a multiple of y_cols.
 *   epoch: ONE int32 on the device, read by the kernel (a recorded launch sees a new epoch at replay).
 *   table: K rows of 2 * C + 6 int32 on the device, 0 <= K <= 64, a row = src[C], flip[C], axis[3], sign[3]:
 *   src[c] in [0, C), flip[c] in {0, 1, 2}, axis a permutation of 0..2, sign +-1.  K == 0 with table NULL: no channel
 *   transform.  The CONTENT of the table is validated by the caller (hip_ops.Augment, before upload); the entry point
 *   checks sizes only, and the kernel reads nothing outside a row whatever the table holds (a src outside [0, C) is
 *   taken as c, an axis outside 0..2 as a, flip is taken mod 4 with 3 as 0).
 *   Random numbers: w = philox4x32_10(counter, key) as seld_dropout_fwd uses it (counter = (low, high, 0, 0), key =
 *   (low, high) of the 64-bit values), words w[0..3] in the order (c0, c1, c2, c3);
 *       key = seed        counter = (uint64)epoch << 34 | (uint64)p << 2 | g        (mod 2^64)
 *   for the sample at position p and the group g in {0, 1, 2}; int(w, n) = ((uint64)w * n) >> 32 is an integer in
 *   [0, n); coin(w) = u01(w) < p_swap in fp32, u01(w) = (float)(w >> 8) * 2^-24.  The draws are functions of (seed,
 *   epoch, p) alone: not of B, count, the cursor-against-start form of the call, or the grid.  The dropout stream is
 *   not touched.
 *   g = 0, channel transform: applied iff K > 0 and coin(w[1]); k = int(w[0], K); with the row k of the table
 *       x'[c, f, t] = flipop(flip[c], x[src[c], f, t])
 *       flipop(0, v) = v;  flipop(1, v) = -v;  flipop(2, v) = v <= 0 ? v + PI_F : v - PI_F, PI_F = (float)M_PI, one fp32
 *       addition: a raw phase in (-pi, pi] turned by pi, staying in that interval
 *       location'(s, a) = (float)sign[a] * location(s, axis[a]);  activity copied
 *   g = 1, frequency masks: for m < n_fmask, width = int(w[2m], f_max + 1), first = int(w[2m + 1], F - width + 1),
 *       x'[:, first : first + width, :] = fill
 *   g = 2, time masks: the same over T with n_tmask, t_max: x'[:, :, first : first + width] = fill
 *   Masks come after the channel transform and cover every channel; targets are not masked.
 *   16-byte loads and stores when T % 4 == 0 and x_all and out_x are 16-byte aligned (a float4 then lies in one
 *   (c, f) row), single floats otherwise; targets whose sample draws no transform move as in seld_gather_rows.
 *   SELD_EINVAL: whatever seld_gather_rows refuses; n_index > 2^32; epoch NULL; K outside [0, 64]; table NULL with
 *   K > 0 or given with K == 0; C outside [1, 16]; F or T < 1 (checked with or without the x pair); row_x != C * F * T;
 *   y_cols < 4, no multiple of 4 or no divisor of row_y (with the y pair); p_swap outside [0, 1]; n_fmask or n_tmask
 *   outside {0, 1, 2}; f_max outside [0, F]; t_max outside [0, T].  SELD_EUNSUPPORTED: a row of 2^31 floats or more.
 *   Nothing is launched on refusal.
 * seld_gather_rows_rot is seld_gather_rows with a per-sample ROTATION of the sound field applied on the way, for
 * predictors whose directional channels are intensity-vector components (seld_spatial_features, kind IV, or kind
 * LOGPOWER_IV in the quaternion layout): a real 3-vector per (f, t) that a rotation R of the sound field turns into
 * R times itself, the normaliser E being invariant.  Addressing, zero-fill of invalid positions, untouched rows
 * [count, B), geometry (C, F, T, y_cols), epoch, seed, the counter and the masks are those of seld_gather_rows_aug; one
 * launch, recordable.
 *   triples: n_triples in [1, 5] channel triples (cx, cy, cz), the x, y and z component of one intensity vector each,
 *   passed BY VALUE, 4 bits per entry: entry 3 * k + a (a = 0, 1, 2 for cx, cy, cz of triple k) in bits
 *   [4 * (3k + a), 4 * (3k + a) + 4).  The entries are distinct and inside [0, C); bits above the last entry are 0.
 *   Every channel outside the triples is copied.
 *   g = 3, rotation (a group seld_gather_rows_aug does not draw; g = 0 is not drawn here):
 *       w = philox4x32_10(counter | 3, seed);  applied iff u01(w[1]) < p_rot
 *       u = u01(w[0]);  (s, c) = sincospif(2 * u)   (2 * u is exact in fp32: no argument-reduction error)
 *       mirror = rot_mirror && (w[2] >> 31);  zflip = rot_zflip && (w[3] >> 31)
 *       R = diag(1, mirror ? -1 : 1, zflip ? -1 : 1) . [[c, -s, 0], [s, c, 0], [0, 0, 1]]
 *     a rotation about the vertical axis by a uniform angle, optionally mirrored in y and in z.
 *   matrices (nullable): (count, 9) fp32 on the device, row-major.  Sample b then takes matrices[b] as R whatever
 *     p_rot says, and group 3 is not drawn.  The matrix is applied as given: orthogonality is the caller's business.
 *   A rotated sample, per triple and (f, t), and per label slot s:
 *       x'[c_a] = fma(R[a][2], x[cz], fma(R[a][1], x[cy], R[a][0] * x[cx]))                          a = 0, 1, 2
 *       location'(s, a) = fma(R[a][2], location(s, 2), fma(R[a][1], location(s, 1), R[a][0] * location(s, 0)))
 *     in fp32; activity copied.  A sample that draws no rotation, and every channel outside the triples, moves as bits.
 *   g = 1, g = 2: the masks of seld_gather_rows_aug, after the rotation, over every channel, filled with `fill`.
 *   Every predictor byte is read once and written once: a lane that owns a 16-byte piece of a triple loads its three
 *   channels and stores three.  16-byte accesses when T % 4 == 0 and x_all and out_x are 16-byte aligned, single floats
 *   otherwise.  No LDS, no atomics: results are run-to-run identical.
 *   SELD_EINVAL: whatever seld_gather_rows_aug refuses of the arguments they share (epoch NULL among them, with or
 *   without matrices; count > B); n_triples outside [1, 5]; 3 * n_triples > C; an entry of triples outside [0, C) or
 *   given twice, a set bit above the last entry; p_rot outside [0, 1].  SELD_EUNSUPPORTED: a row of 2^31 floats or
 *   more.  Nothing is launched on refusal.
 * seld_gather_rows_polar is seld_gather_rows_rot for predictors stored as [magnitude channels | phase channels]: magnitude
 * and phase of one STFT bin are one complex number and the STFT is linear, so a rotation R of the FOA waveform turns the
 * complex 3-vector Z = (X, Y, Z) of every (f, t) into R Z; W stays.  Addressing, cursor / start / count / stride,
 * zero-fill of invalid positions, untouched rows [count, B), geometry (C, F, T, y_cols), epoch, seed, the counter, group
 * 3 (the rotation draw, word for word), groups 1 and 2 (the masks), the `matrices` override and the label rotation (the
 * same fma order) are those of seld_gather_rows_rot; one launch, recordable.
 *   groups: n_groups in [1, 2] channel groups (mx, my, mz, px, py, pz), magnitude and phase of the x, y and z channel
 *   of one microphone, passed BY VALUE, 4 bits per entry: entry 6 * k + e (e = 0..5 in the order above) in bits
 *   [4 * (6k + e), 4 * (6k + e) + 4).  The entries are distinct and inside [0, C); bits above the last entry are 0.
 *   Every other channel, magnitude and phase of W among them, is copied as bits.
 *   stats (nullable): 4 fp32 on the device, (mean_m, sd_m, mean_p, sd_p): the predictors hold (magnitude - mean_m) / sd_m
 *   and (phase - mean_p) / sd_p (seld_group_standardize over the two halves).  The kernel reads them; NULL: raw
 *   magnitude and phase.  Their CONTENT is the caller's business (finite, sd > 0: hip_ops.gather_rows_polar checks it
 *   once per tensor), like the content of a transform table.
 *   A rotated sample, per group and (f, t), in fp32 (j = x, y, z; a = 0, 1, 2):
 *       m_j  = fma(x[m_j], sd_m, mean_m)         phi_j = fma(x[p_j], sd_p, mean_p)
 *       (s_j, c_j) = sincosf(phi_j);   re_j = m_j * c_j;   im_j = m_j * s_j
 *       re'_a = fma(R[a][2], re_z, fma(R[a][1], re_y, R[a][0] * re_x))           im'_a alike
 *       m'_a = sqrtf(fma(im'_a, im'_a, re'_a * re'_a))       phi'_a = atan2f(im'_a, re'_a)
 *       x'[m_a] = __fdiv_rn(m'_a - mean_m, sd_m)             x'[p_a] = __fdiv_rn(phi'_a - mean_p, sd_p)
 *     With stats NULL the two affine steps on either side are SKIPPED (not computed with 0 and 1): x'[m_a] = m'_a >= 0 and
 *     x'[p_a] = phi'_a, which lies in [-PI_F, PI_F]; atan2f(0, 0) = 0 as numpy's angle.  Labels as seld_gather_rows_rot.
 *     A sample that draws no rotation, and every channel outside the groups, moves as bits.
 *   g = 1, g = 2: the masks of seld_gather_rows_aug, after the rotation, over every channel, filled with `fill`.
 *   Every predictor byte is read once and written once: a lane that owns a 16-byte piece of a group loads its six
 *   channels and stores six; group tiles are numbered before the tiles of the other channels.  16-byte accesses when
 *   T % 4 == 0 and x_all and out_x are 16-byte aligned, single floats otherwise.  No LDS, no atomics: results are
 *   run-to-run identical.
 *   SELD_EINVAL: whatever seld_gather_rows_rot refuses of the arguments they share; n_groups outside [1, 2];
 *   6 * n_groups > C; an entry of groups outside [0, C) or given twice, a set bit above the last entry.
 *   SELD_EUNSUPPORTED: a row of 2^31 floats or more.  Nothing is launched on refusal.
 * seld_target_occupancy, once per resident target array (outside any capture): target rows are (T_out, y_cols) with
 * y_cols = 4 * n_sed, n_sed = classes * overlaps, the slot of (class c, place o) being c * overlaps + o (what
 * seld_encode_events writes).  A slot is ACTIVE iff its activity > 0.5f (a NaN is inactive).
 *     occ[r, c] = max over the frames of row r of the number of active slots of class c        occ: (n_rows, classes) uint8
 *   One launch, one writer per byte, no atomics.  SELD_EINVAL: a NULL pointer, a non-positive size, y_cols no positive
 *   multiple of 4 * overlaps, row_y no multiple of y_cols.  SELD_EUNSUPPORTED: classes > 64, overlaps > 8, row_y >= 2^31.
 *   Nothing is launched on refusal.
 * seld_gather_rows_mix is seld_gather_rows with a SECOND clip mixed into a sample on the way, for predictors stored as
 * [magnitude channels | phase channels]: the STFT is linear, so the mixture a + g b of two recordings has the spectrum
 * z_A + g z_B bin by bin; on these predictors mixing in the loader equals mixing the waveforms.  Addressing, cursor / start
 * / count / stride, zero-fill of invalid positions, untouched rows [count, B), geometry (C, F, T, y_cols), epoch, seed, the
 * counter, groups 1 and 2 (the masks, after the mix, over every channel), the 16-byte / scalar path rule and `stats` (NULL:
 * both affine steps are skipped) are those of seld_gather_rows_polar; one launch, recordable.
 *   Layout: C is even; channel c < C / 2 is a magnitude and channel c + C / 2 its phase.  Every pair is mixed, W like
 *   any other: a mixed sample has no channel that is copied.
 *   The draw.  Groups 0..3 of a sample's counter are taken, so the mix has a key of its own:
 *       w = philox4x32_10(counter with g = 0, seed ^ 0x9E3779B97F4A7C15)
 *       drawn iff p_mix > 0, n_index > 1 and u01(w[1]) < p_mix
 *       p2 = (p + 1 + int(w[0], n_index - 1)) mod n_index      the partner POSITION: never p; any position of `index`
 *       g  = fma(u01(w[2]), gain_hi - gain_lo, gain_lo)
 *   partners, gains (nullable, both or neither): `count` int64 and `count` fp32 on the device.  Sample b then takes
 *   p2 = partners[b] and g = gains[b] and nothing is drawn; p2 outside [0, n_index) means no mix.  Their content is the
 *   caller's business, as that of `matrices` is.
 *   A drawn sample IS mixed iff its partner row r2 = index[p2] lies in [0, n_rows) and, with `occupancy` (nullable: the
 *   table of seld_target_occupancy over y_all with the same overlaps),  occ[r, c] + occ[r2, c] <= overlaps  for every
 *   class c: no frame can then hold more events of a class than it has slots, so no label is ever dropped (the test is
 *   per clip, not per frame: conservative).  A sample that is not mixed moves as bits, masks aside.
 *   A mixed sample, per pair (m, p) and (f, t), in fp32 without contraction (S = A, the sample, and B, its partner):
 *       m_S = fma(x_S[m], sd_m, mean_m)       phi_S = fma(x_S[p], sd_p, mean_p)
 *       (s_S, c_S) = sincosf(phi_S);   re_S = m_S * c_S;   im_S = m_S * s_S
 *       re = fma(g, re_B, re_A)               im = fma(g, im_B, im_A)
 *       m' = sqrtf(fma(im, im, re * re))      phi' = atan2f(im, re)
 *       x'[m] = __fdiv_rn(m' - mean_m, sd_m)  x'[p] = __fdiv_rn(phi' - mean_p, sd_p)
 *     (with stats NULL x'[m] = m' and x'[p] = phi').  A lane that owns a 16-byte piece of a pair loads it from both
 *     channels of both rows, four loads ahead of two stores; a frequency row under a mask is read from neither row.
 *   Targets of a mixed sample, per (frame, class): the LIST is A's active slots in slot order, then B's.  Output slot k of
 *   the class takes the activity and the three location values of entry k as bits; slots behind the list get +0.0f in
 *   all four; entries from `overlaps` on are dropped (without `occupancy` that truncation is the defined result).
 *   Locations are not scaled by g.  One writer per element, no LDS, no atomics: results are run-to-run identical.
 *   SELD_EINVAL: whatever seld_gather_rows_polar refuses of the arguments they share; C odd; overlaps < 1; y_cols no
 *   multiple of 4 * overlaps (with the y pair or with occupancy, which both read y_cols as 4 * classes * overlaps); p_mix
 *   outside [0, 1]; gains that are not finite or not 0 < gain_lo <= gain_hi; one of partners / gains without the other.
 *   SELD_EUNSUPPORTED: classes > 64, overlaps > 8, a row of 2^31 floats or more.  Nothing is launched on refusal.
 * seld_epoch_step_end, one thread, as the last launch of a step:
 *     mean[0] += (loss[0] - mean[0]) / (float)(cursor[0] + 1);   cursor[0] += 1          (fp32: the epoch loop's
 *   running mean of the loss, train.py:559, in the form train.main takes it)
 *   loss, mean: device fp32 scalars; cursor: the device int32 above.  An epoch is then n replays with no host-to-device
 *   traffic and no read-back.  SELD_EINVAL: a NULL pointer.
 * ------------------------------------------------------------------------------------------ */
int seld_gather_rows(const float* x_all, int64_t row_x, float* out_x, const float* y_all, int64_t row_y, float* out_y,
                     const int64_t* index, int64_t n_index, int64_t n_rows, const int32_t* cursor, int64_t cursor_stride,
                     int64_t start, int32_t B, int32_t count, void* stream);
int seld_gather_rows_aug(const float* x_all, int64_t row_x, float* out_x, const float* y_all, int64_t row_y, float* out_y,
                         const int64_t* index, int64_t n_index, int64_t n_rows, const int32_t* cursor, int64_t cursor_stride,
                         int64_t start, int32_t B, int32_t count, int32_t C, int32_t F, int32_t T, int32_t y_cols,
                         const int32_t* epoch, uint64_t seed, const int32_t* table, int32_t K, float p_swap, int32_t n_fmask,
                         int32_t f_max, int32_t n_tmask, int32_t t_max, float fill, void* stream);
int seld_gather_rows_rot(const float* x_all, int64_t row_x, float* out_x, const float* y_all, int64_t row_y, float* out_y,
                         const int64_t* index, int64_t n_index, int64_t n_rows, const int32_t* cursor, int64_t cursor_stride,
                         int64_t start, int32_t B, int32_t count, int32_t C, int32_t F, int32_t T, int32_t y_cols,
                         const int32_t* epoch, uint64_t seed, uint64_t triples, int32_t n_triples, float p_rot,
                         int32_t rot_mirror, int32_t rot_zflip, const float* matrices, int32_t n_fmask, int32_t f_max,
                         int32_t n_tmask, int32_t t_max, float fill, void* stream);
int seld_gather_rows_polar(const float* x_all, int64_t row_x, float* out_x, const float* y_all, int64_t row_y,
                           float* out_y, const int64_t* index, int64_t n_index, int64_t n_rows, const int32_t* cursor,
                           int64_t cursor_stride, int64_t start, int32_t B, int32_t count, int32_t C, int32_t F, int32_t T,
                           int32_t y_cols, const int32_t* epoch, uint64_t seed, uint64_t groups, int32_t n_groups,
                           const float* stats, float p_rot, int32_t rot_mirror, int32_t rot_zflip, const float* matrices,
                           int32_t n_fmask, int32_t f_max, int32_t n_tmask, int32_t t_max, float fill, void* stream);
int seld_target_occupancy(const float* y_all, int64_t n_rows, int64_t row_y, int32_t y_cols, int32_t overlaps, uint8_t* occ,
                          void* stream);
int seld_gather_rows_mix(const float* x_all, int64_t row_x, float* out_x, const float* y_all, int64_t row_y, float* out_y,
                         const int64_t* index, int64_t n_index, int64_t n_rows, const int32_t* cursor, int64_t cursor_stride,
                         int64_t start, int32_t B, int32_t count, int32_t C, int32_t F, int32_t T, int32_t y_cols,
                         const int32_t* epoch, uint64_t seed, int32_t overlaps, const float* stats, float p_mix, float gain_lo,
                         float gain_hi, const int64_t* partners, const float* gains, const uint8_t* occupancy, int32_t n_fmask,
                         int32_t f_max, int32_t n_tmask, int32_t t_max, float fill, void* stream);
int seld_epoch_step_end(const float* loss, float* mean, int32_t* cursor, void* stream);

/* ------------------------------------------------------------------------------------------
 * Whole-recording inference (csrc/ensemble.hip): sliding windows over resident recordings, each window under every row
 * of a transform table, and the members' outputs combined into one track per recording.  Neither entry point allocates
 * or synchronises; both can be recorded in a HIP graph; a refused call launches nothing and writes nothing.
 *
 * Notation: recordings x (R, C, F, L) fp32; windows of T input frames every `hop` frames, S per recording; a transform
 * table of K rows of 2 * C + 6 int32 in the layout of seld_gather_rows_aug (src[C], flip[C], axis[3], sign[3]), its
 * CONTENT validated by the caller as there.  K == 0 with table NULL is the identity alone and counts as K = 1 below.
 * Members are numbered m = (r * S + s) * K + k.
 *
 * seld_window_batch cuts and transforms the members [m0, m0 + count) in one launch.  For b < count, m = m0 + b:
 *     out[b, c, f, j] = flipop(flip_k[c], t < L ? x[r, src_k[c], f, t] : 0),      t = s * hop + j,  0 <= j < T
 *   flipop as documented for seld_gather_rows_aug, applied to the padding zero as well (flip 2 makes it PI_F): the
 *   bytes of seld_segment followed by the training transform.  out is (B, C, F, T); rows [count, B) are not touched.  A
 *   src outside [0, C) is taken as c, flip is taken mod 4 with 3 as 0.
 *   One read and one write per output byte.  16-byte loads and stores when T, hop and L are multiples of 4 and x and
 *   out are 16-byte aligned (a float4 then lies in one (c, f) row and wholly inside or wholly past L), single floats
 *   otherwise.
 *   SELD_EINVAL: x or out NULL; R, F, L, T, hop, S, B or count < 1; C outside [1, 16]; count > B; count > 65535;
 *   K outside [0, 64]; table NULL with K > 0 or given with K == 0; m0 < 0 or m0 + count > R * S * K.
 *   SELD_EUNSUPPORTED: C * F * T or C * F * L of 2^31 floats or more.
 *
 * seld_ensemble_combine takes the members' outputs sed (M, T_out, n) and doa (M, T_out, 3 * n), M = R * S * K,
 * n = classes * overlaps <= 64, slot c * O + o (O = overlaps) and axis a at doa[.., 3 * (c * O + o) + a] (the model's
 * and the loss's layout); hop_out, the hop in output frames; frames, the output frames of a recording; win, T_out
 * positive finite fp32 weights on the device (validated by the caller); the table (C its channel count: the row
 * stride; ignored with K == 0); align, 0 or 1.  It writes out_sed (R, frames, n), out_doa (R, frames, 3 * n) and, if
 * non-NULL, perm (M, T_out, classes) int32.  For each cell (r, t, c), t < frames:
 *   - the covering windows are the s < S with 0 <= j = t - s * hop_out < T_out; the members of the cell are those
 *     windows x every k, visited s ascending, then k ascending;
 *   - a member's values are mapped back through its row:  p_m[o] = sed_m[j, c * O + o]  and
 *         q_m[o][axis_k[a]] = (float)sign_k[a] * doa_m[j, 3 * (c * O + o) + a]
 *     the inverse of location'[a] = sign[a] * location[axis[a]] (whatever the row holds, nothing outside it is read);
 *   - the anchor A is the member (s*, k = 0), s* the covering window with the largest win[j], the lowest s of equals;
 *   - with align and O > 1 every member picks a slot permutation pi, output slot o taking member slot pi(o), that
 *     minimises  cost(pi) = (P[0][pi0] + P[1][pi1]) + P[2][pi2]  (the terms of missing slots absent) with
 *         P[o][i] = (((p_m[i] - p_A[o])^2 + (q_m[i][0] - q_A[o][0])^2) + (q_m[i][1] - q_A[o][1])^2) + (q_m[i][2] - q_A[o][2])^2
 *     in fp32, products and sums rounded separately.  Permutations are numbered in lexicographic order as for
 *     seld_loss_pit_fwd_bwd; the search starts from the identity and moves on `<` only: ties and NaN costs keep the
 *     lower index.  Without align, or with O == 1, pi is the identity (index 0);
 *   - out[o] = (sum_m w_m * v_m[pi_m(o)]) / (sum_m w_m),  w_m = win[j], for the activity and each of the three axes:
 *     fp32 products and sums in member order from 0, one division.  One writer per element, no atomics: two runs give
 *     the same bytes.  A frame that no window covers is written as zeros.
 *   perm[m, j, c] is the chosen index, and -1 where s * hop_out + j >= frames (every entry of perm is written).
 *   One launch, one thread per cell, contiguous reads of a frame's n / 3 * n values, no LDS.
 *   SELD_EINVAL: sed, doa, win, out_sed or out_doa NULL; R, S, T_out, hop_out, frames, classes or overlaps < 1;
 *   K outside [0, 64]; table NULL with K > 0 or given with K == 0; C outside [1, 16] with K > 0; align not 0 or 1.
 *   SELD_EUNSUPPORTED: classes * overlaps > 64; align with overlaps > 3; 2^31 workgroups or more.
 * ------------------------------------------------------------------------------------------ */
int seld_window_batch(const float* x, int64_t R, int32_t C, int32_t F, int32_t L, int32_t T, int32_t hop, int32_t S,
                      const int32_t* table, int32_t K, int64_t m0, int32_t B, int32_t count, float* out, void* stream);
int seld_ensemble_combine(const float* sed, const float* doa, int64_t R, int32_t S, int32_t K, int32_t T_out,
                          int32_t hop_out, int32_t frames, int32_t classes, int32_t overlaps, const float* win,
                          const int32_t* table, int32_t C, int32_t align, float* out_sed, float* out_doa, int32_t* perm,
                          void* stream);

/* ------------------------------------------------------------------------------------------
 * Track post-processing (csrc/smooth.hip): what SELD systems apply between the network's frame-wise outputs and the
 * event list -- a median filter on the activity, two thresholds with hysteresis, gap filling, a minimum duration and
 * one DOA per event -- and the event list of any track.  Nothing here allocates; a refused call launches nothing and
 * writes nothing.
 *
 * Notation: a track is sed (R, T, n) and doa (R, T, 3 * n), contiguous fp32, n = classes * overlaps: the layout of the
 * model, of seld_ensemble_combine and of seld_decode_*.  A COLUMN is one (r, j), j < n, over its T frames; its DOA at
 * frame t is doa[r, t, 3j : 3j + 3].  A RUN is a maximal stretch of frames of a column with one value of a flag.
 *
 * seld_smooth_tracks writes out_sed (R, T, n), out_doa (R, T, 3 * n) and, if non-NULL, out_prob (R, T, n), in ONE launch
 * on `stream`, no host read: it can be recorded in a HIP graph.  Per column, independently of every other:
 *   1. p[t] = the median of sed over the frames t - h .. t + h, h = (median - 1) / 2, frame indices clamped to
 *      [0, T - 1] (edge replication inside the recording: scipy.ndimage.median_filter(mode='nearest') along time).
 *      median is odd, 1 <= median <= SELD_SMOOTH_MAX_MEDIAN; median == 1 gives p = sed.  The median is an element of
 *      the window, so p is exact.  Nothing is promised for NaN.  out_prob = p.
 *   2. hysteresis: c[t] = p[t] > off; a run of c = 1 is kept iff it holds a frame with p[t] > on.  Both comparisons are
 *      strict (with on = off = 0.5 and p in [0, 1] this is the decoder's rint, for which 0.5 is off) and in fp32: `on`
 *      and `off` are floats.  The result is a1.
 *   3. gap fill: a run of a1 = 0 with an active frame on both sides (so it touches neither frame 0 nor frame T - 1) of
 *      at most max_gap frames becomes active.  The result is a2.
 *   4. minimum duration: a run of a2 = 1 of fewer than min_frames frames becomes inactive, at a recording's ends as
 *      anywhere else.  The result is a3.
 *   5. out_sed[t] = a3[t] ? 1.0f : 0.0f.
 *   6. doa_mode SELD_SMOOTH_DOA_FRAME: out_doa = doa everywhere.  SELD_SMOOTH_DOA_MEAN (w = 1) and
 *      SELD_SMOOTH_DOA_WEIGHTED (w = p[t]): every run of a3 = 1 gets, per axis, (float)(sum w[t] * d[t] / sum w[t]) over
 *      ITS frames -- products and sums in double, in a fixed order (frame order inside each of the kernel's chunks of
 *      consecutive frames, then the chunks in order), one division, one rounding to float; no term from outside the run
 *      enters, so each sum is within run length * 2^-53 of exact, relatively.  sum w > 0: a surviving run holds a frame
 *      with p > on >= 0.  The value goes to every frame of the run; frames with a3 = 0 copy doa.
 *   One writer per element, no atomics: two runs give the same bytes.  out_* may not alias the inputs.
 *   One 256-thread workgroup per column with the column in LDS (9 T + 12352 bytes); the rules are scans over frames.
 *   SELD_EINVAL: sed, doa, out_sed or out_doa NULL; R, T or n < 1; median even or outside 1 .. SELD_SMOOTH_MAX_MEDIAN;
 *   on or off not finite or not 0 <= off <= on <= 1; min_frames < 1; max_gap < 0; an unknown doa_mode.
 *   SELD_EUNSUPPORTED: T > SELD_SMOOTH_MAX_FRAMES (the column no longer fits the CU's LDS); R * n of 2^31 or more.
 *
 * seld_track_events_*: the event list of a track, by the two calls of seld_decode_* with one 8-byte device-to-host read
 * between them.  A frame of a column is active when sed > 0.5: for the 0/1 output above and for probabilities in [0, 1]
 * that is the decoder's rule; outside [0, 1] it is NOT rint (1.5 rounds to 2 and is active either way, but -0.6 is
 * active for the decoder and inactive here), and the decoder's frame-sum rule is not applied.  Every run of active frames
 * gives one row of 8 doubles
 *     { recording, class = j / overlaps, slot = j % overlaps, onset, offset (exclusive), x, y, z }
 *   x, y, z = (sum of the run's DOAs in double, frame order) / length * max_loc_value, all in double.  Rows are ordered
 *   recording-major, then column, then onset; rec_offsets (R + 1) int64, CSR style.
 *   seld_track_events_workspace  bytes of workspace both calls need (0 for a refused shape)
 *   seld_track_events_count      reads sed once; leaves the row count E as an int64 in the first 8 bytes of the workspace
 *   seld_track_events_write      takes the SAME workspace, untouched since the count call on the same sed and shape,
 *                                rows (capacity, 8) and rec_offsets (R + 1); capacity >= E; rows beyond capacity are
 *                                not written; rows may be NULL when capacity is 0
 *   No atomics.  SELD_EINVAL: a NULL pointer, a size < 1, a negative capacity; SELD_EUNSUPPORTED: R * n * ceil(T / 64)
 *   of 2^31 or more; SELD_EWORKSPACE: a missing or short workspace.
 * ------------------------------------------------------------------------------------------ */
#define SELD_SMOOTH_MAX_MEDIAN 31
#define SELD_SMOOTH_MAX_FRAMES 16384   /* 27 minutes of 100 ms frames */
#define SELD_SMOOTH_DOA_FRAME 0
#define SELD_SMOOTH_DOA_MEAN 1
#define SELD_SMOOTH_DOA_WEIGHTED 2
int seld_smooth_tracks(const float* sed, const float* doa, int64_t R, int32_t T, int32_t n, int32_t median, float on,
                       float off, int32_t min_frames, int32_t max_gap, int32_t doa_mode, float* out_sed, float* out_doa,
                       float* out_prob /* may be NULL */, void* stream);
size_t seld_track_events_workspace(int64_t R, int32_t T, int32_t n);
int seld_track_events_count(const float* sed, int64_t R, int32_t T, int32_t n, void* workspace, size_t workspace_bytes,
                            void* stream);
int seld_track_events_write(const float* sed, const float* doa, int64_t R, int32_t T, int32_t classes, int32_t overlaps,
                            double max_loc_value, const void* workspace, size_t workspace_bytes, double* rows,
                            int64_t capacity, int64_t* rec_offsets, void* stream);

/* ------------------------------------------------------------------------------------------
 * Squeeze-and-excitation (csrc/squeeze_excite.hip): a per-sample channel gate.  x is (N, C, S) fp32 contiguous, S >= 1 the
 * product of the spatial extents.  A in {1, 4, 8} hypercomplex components, C % A == 0, Cg = C / A gated channels; the
 * component blocks are contiguous along the channel axis (channel c = k Cg + g), so ONE gate multiplies a whole
 * (dual) quaternion by a real scalar.  Hd >= 1 hidden units.  W1 (Hd, Cg), b1 (Hd), W2 (Cg, Hd), b2 (Cg), row-major.
 *
 *   z[n,g]   = (1 / (A S)) sum_k sum_s x[n, k Cg + g, s]
 *   h[n,r]   = relu(sum_g W1[r,g] z[n,g] + b1[r])
 *   s[n,g]   = sigmoid(sum_r W2[g,r] h[n,r] + b2[g])
 *   y[n,c,:] = x[n,c,:] s[n, c mod Cg]
 *
 *   q[n,g]   = sum_k sum_s dy x        dp2 = q s (1 - s)        dh = (W2^T dp2) [h > 0]
 *   dW2 = sum_n dp2 (x) h    db2 = sum_n dp2    dW1 = sum_n dh (x) z    db1 = sum_n dh    dz = W1^T dh
 *   dx[n,c,:] = dy[n,c,:] s[n,g] + dz[n,g] / (A S)
 *
 * 1 / (A S) is ONE float, (float)(1.0 / ((double)A * S)), multiplied in; the sigmoid is 1.0f / (1.0f + expf(-p)).
 * The six calls, each on `stream`, no host read, no allocation (they record into a HIP graph):
 *   seld_se_squeeze      rowsum[row] = sum_s x[row, s] for the rows = N C rows of S floats
 *   seld_se_excite_fwd   folds the A row sums of a gated channel (k = 0, 1, ...), writes z (N, Cg), h (N, Hd), s (N, Cg)
 *   seld_se_scale        y = x s
 *   seld_se_bwd_reduce   q[row] = sum_s dy[row, s] x[row, s]
 *   seld_se_excite_bwd   folds q like the row sums; writes dp2 (N, Cg), dh (N, Hd), dz (N, Cg) and the four parameter
 *                        gradients, each summed over n = 0, 1, ... in order by one thread; accumulate != 0 adds the sum
 *                        to what dw1 / db1 / dw2 / db2 hold (an optimiser's gradient slots), 0 overwrites
 *   seld_se_bwd_apply    dx = dy s + dz / (A S)
 * The two calls that sum (squeeze, bwd_reduce) give every row one owner: the row form (one wave per row) for
 * S < SELD_SE_BLOCK_MIN_S and the block form (one 256-thread workgroup per row) from there on.  The two that write (scale,
 * bwd_apply) take the chunk form: one wave per 256 floats of a row.  All use 16-byte accesses between a row's head and
 * tail whatever S % 4 is; when the tensors of one call sit at different offsets from a 16-byte boundary they walk single
 * elements (seld_se_kernel_label: "<op>_<row|block|chunk>_kernel[x4|x1]", same_phase != 0 for equal offsets).  Row and
 * element offsets are 64-bit.  There is no float atomic: every sum has one owner and a fixed order
 * (csrc/squeeze_excite.hip states it), so two runs give the same bytes with and without SELD_DETERMINISTIC.  Outputs may
 * not alias inputs.
 *   SELD_EINVAL: a NULL pointer, an extent < 1, A outside {1, 4, 8}, C % A != 0.
 *   SELD_EUNSUPPORTED (nothing is launched or written): Cg > SELD_SE_MAX_GATED or Hd > SELD_SE_MAX_HIDDEN -- z / dp2 and
 *   h / dh of a sample are held in 20 KiB of LDS; scale / bwd_apply on 2^32 chunks (4 TiB of floats) or more.
 * ------------------------------------------------------------------------------------------ */
#define SELD_SE_MAX_GATED 4096
#define SELD_SE_MAX_HIDDEN 1024
#define SELD_SE_BLOCK_MIN_S 1024
#define SELD_SE_SQUEEZE 0              /* seld_se_kernel_label(op, ...) */
#define SELD_SE_SCALE 1
#define SELD_SE_BWD_REDUCE 2
#define SELD_SE_BWD_APPLY 3
int seld_se_squeeze(const float* x, int64_t rows, int32_t S, float* rowsum, void* stream);
int seld_se_excite_fwd(const float* rowsum, int32_t N, int32_t C, int32_t S, int32_t A, int32_t Hd, const float* w1,
                       const float* b1, const float* w2, const float* b2, float* z, float* h, float* s, void* stream);
int seld_se_scale(const float* x, int32_t N, int32_t C, int32_t S, int32_t A, const float* s, float* y, void* stream);
int seld_se_bwd_reduce(const float* dy, const float* x, int64_t rows, int32_t S, float* q, void* stream);
int seld_se_excite_bwd(const float* q, int32_t N, int32_t C, int32_t A, int32_t Hd, const float* w1, const float* w2,
                       const float* z, const float* h, const float* s, float* dp2, float* dh, float* dz, float* dw1,
                       float* db1, float* dw2, float* db2, int32_t accumulate, void* stream);
int seld_se_bwd_apply(const float* dy, int32_t N, int32_t C, int32_t S, int32_t A, const float* s, const float* dz,
                      float* dx, void* stream);
int seld_se_kernel_label(int32_t op, int32_t S, int32_t same_phase, char* buf, int32_t buflen);

/* ------------------------------------------------------------------------------------------
 * Temporal attention (csrc/temporal_attention.hip): the single-head attention core of the TCN's "AT" blocks, flash style,
 * on ONE projected tensor qkv (N, 2K + V, T) = [q (K) | k (K) | v (V)] along the channels, fp32 contiguous, T contiguous.
 * The key width K and the value width V are independent, 1 <= K, V <= SELD_AT_MAX_WIDTH.
 *
 *   score[n,t,s]   = (sum_d q[n,d,t] k[n,d,s]) / sqrt(K)
 *   allowed(n,t,s) = kind(t, s) && s < len[n]
 *                    SELD_AT_NONE: true      SELD_AT_CAUSAL: s <= t      SELD_AT_BAND: |t - s| <= band
 *   p[n,t,:]       = softmax of score[n,t,:] over the allowed s; an excluded key has weight EXACTLY 0 (this is not the
 *                    -1e9 convention of seld_mha_*_ex, where a fully masked row attends uniformly)
 *   read[n,:,t]    = sum_s p[n,t,s] v[n,:,s]            (N, V, T)
 *   lse[n,t]       = log sum_{allowed s} exp(score[n,t,s])       (N, T)
 *
 * lengths: an optional int32 device array of N valid lengths, each clamped by the kernels into [1, T]; NULL: T.  band is
 * read for SELD_AT_BAND only (but must never be negative).  A row with no allowed key can arise only from SELD_AT_BAND
 * together with lengths (t - band >= len[n]): it gives read = 0 and lse = +inf and contributes nothing to any gradient.
 *
 *   delta[n,t] = sum_d dread[n,d,t] read[n,d,t]         dp[n,t,s] = sum_d dread[n,d,t] v[n,d,s]
 *   ds = p (dp - delta) / sqrt(K)      dq[n,:,t] = sum_s ds k[n,:,s]      dk[n,:,s] = sum_t ds q[n,:,t]
 *   dv[n,:,s] = sum_t p dread[n,:,t]                    dqkv = [dq | dk | dv], every element written
 *
 * seld_at_fwd is one launch; seld_at_bwd three (delta into the workspace of seld_at_bwd_workspace(N, T) bytes, a dq kernel
 * that owns query tiles, a dk/dv kernel that owns key tiles).  No atomics: a repeated call gives the same bytes.  All on
 * `stream`, no host read, no allocation: the calls record into a HIP graph.  Every kernel loops only over the tiles of the
 * opposite index that the mask allows for its own tile; tiles the mask excludes are never loaded.
 * Forms (seld_at_kernel_label: "at_<fwd|bwd_dq|bwd_dkv>_mfma_kernel<K,V>" or "..._valu_kernel<W>", W = max(K, V) rounded up to
 * 8 / 16 / 32 / 48 / 64): fp32-MFMA kernels when K and V are each one of 16, 32, 48, 64 and T % 16 == 0 (and
 * SELD_MHA_NO_MFMA is not set); VALU kernels otherwise, and for tensors off a 16-byte boundary.  Element offsets are 64-bit.
 *   SELD_EINVAL: a NULL tensor, a size <= 0, band < 0, an unknown mask kind (for the label: an unknown op, a short buffer).
 *   SELD_EUNSUPPORTED: K or V > SELD_AT_MAX_WIDTH; N * ceil(T / 32) workgroups of 2^31 or more.
 *   SELD_EWORKSPACE: workspace NULL or smaller than seld_at_bwd_workspace(N, T).
 * All are returned before anything is launched or written.  Outputs may not alias inputs.
 * ------------------------------------------------------------------------------------------ */
#define SELD_AT_MAX_WIDTH 64
#define SELD_AT_NONE 0                 /* mask_kind */
#define SELD_AT_CAUSAL 1
#define SELD_AT_BAND 2
#define SELD_AT_FWD 0                  /* seld_at_kernel_label(op, ...) */
#define SELD_AT_BWD_DQ 1
#define SELD_AT_BWD_DKV 2
int seld_at_fwd(const float* qkv, int32_t N, int32_t T, int32_t K, int32_t V, int32_t mask_kind, int32_t band,
                const int32_t* lengths /* may be NULL */, float* read, float* lse, void* stream);
size_t seld_at_bwd_workspace(int32_t N, int32_t T);
int seld_at_bwd(const float* qkv, const float* read, const float* dread, const float* lse, int32_t N, int32_t T, int32_t K,
                int32_t V, int32_t mask_kind, int32_t band, const int32_t* lengths /* may be NULL */, float* dqkv,
                void* workspace, size_t workspace_bytes, void* stream);
int seld_at_kernel_label(int32_t op, int32_t T, int32_t K, int32_t V, char* buf, int32_t buflen);

/* ------------------------------------------------------------------------------------------
 * GRU (csrc/gru.hip): the recurrence of one torch.nn.GRU layer, gate order r | z | n, for 1 or 2 directions (direction 1
 * walks time backwards).  fp32, contiguous.  With gx = x @ W_ih^T + b_ih (seld_hc_linear_fwd; not part of the recurrence):
 *
 *   r  = sigmoid(gx_r + W_hr h + b_hr)
 *   z  = sigmoid(gx_z + W_hz h + b_hz)
 *   n  = tanh(gx_n + r * (W_hn h + b_hn))
 *   h' = (1 - z) * n + z * h
 *
 * seld_gru_pack writes, for every direction, W_hh (3H, H) as the forward kernel's and W_hh^T as the backward kernel's MFMA
 * fragments and b_hh (NULL: zeros), all zero-padded to Hp = H rounded up to 16, into wpack (seld_gru_pack_floats floats):
 * the recurrence calls read the weights from there only, so the two directions' parameters need not be adjacent.
 *
 * seld_gru_fwd, one launch for every direction:
 *   gx (dirs, B, T, 3H), h0 (dirs, B, H) or NULL (zeros)  ->  y (B, T, dirs*H): each direction writes its half, there is
 *   no concatenation; h_n (dirs, B, H); saved, if not NULL, (5, dirs, B, T, H) = r, z, n, W_hn h + b_hn, h_prev, what
 *   seld_gru_bwd reads (seld_gru_saved_floats floats; h_prev is contiguous per direction: it is the x of dW_hh).
 * seld_gru_bwd, one launch for the reverse recurrence of every direction:
 *   dy (B, T, dirs*H), dh_n (dirs, B, H) or NULL, saved  ->  dgx (dirs, B, T, 3H); dgh (dirs, B, T, 3H) = dgx with the n
 *   part multiplied by r; dh0 (dirs, B, H) or NULL.  dh is carried through W_hh^T.
 *   dW_hh = dgh^T @ h_prev and db_hh = column sums of dgh are ONE product over all steps: seld_hc_linear_bwd(SELD_LIN_REAL,
 *   B*T, H, 3H, h_prev, dgh, ...) per direction; dx, dW_ih, db_ih come from the same call on (x, dgx).
 *
 * Form (seld_gru_kernel_label: "gru_<fwd|bwd>_kernel<Hp/16>"): one workgroup per (direction, 16 batch columns) holds
 * W_hh (backward: W_hh^T) in registers for the whole launch as fp32-MFMA fragments, wave w owning hidden units
 * 16w .. 16w+15; h (backward: dgh) is double-buffered in LDS, one barrier per step.  Columns past B are masked.  No
 * grid-wide barrier, no cooperative launch, no atomics: a repeated call gives the same bytes, and a sample gives the same
 * bytes alone as inside a batch.  All on `stream`, no host read, no allocation: the calls record into a HIP graph.
 * 1 <= H <= SELD_GRU_MAX_HIDDEN: the resident form ends where W_hh outgrows one workgroup's registers; larger hidden
 * sizes need the weights streamed or the units split across workgroups, which is not built.
 *   SELD_EINVAL: a NULL required tensor, a size <= 0, dirs outside {1, 2} (for the label: an unknown op, a short buffer).
 *   SELD_EUNSUPPORTED: H > SELD_GRU_MAX_HIDDEN; 5 * dirs * B * T * H (the saved tensors) of 2^31 or more.
 *   SELD_EWORKSPACE: saved smaller than seld_gru_saved_floats(dirs, B, T, H).
 * All are returned before anything is launched or written.  Outputs may not alias inputs.
 * ------------------------------------------------------------------------------------------ */
#define SELD_GRU_MAX_HIDDEN 128
#define SELD_GRU_FWD 0                 /* seld_gru_kernel_label(op, ...) */
#define SELD_GRU_BWD 1
size_t seld_gru_pack_floats(int32_t dirs, int32_t H);      /* 0 for sizes the calls refuse */
int seld_gru_pack(int32_t dirs, int32_t H, const float* w_hh0, const float* w_hh1 /* dirs == 2 */,
                  const float* b_hh0 /* nullable */, const float* b_hh1 /* nullable, as b_hh0 */, float* wpack, void* stream);
size_t seld_gru_saved_floats(int32_t dirs, int32_t B, int32_t T, int32_t H);       /* 0 for sizes the calls refuse */
int seld_gru_fwd(int32_t dirs, int32_t B, int32_t T, int32_t H, const float* gx, const float* wpack,
                 const float* h0 /* nullable */, float* y, float* h_n, float* saved /* nullable */, size_t saved_floats,
                 void* stream);
int seld_gru_bwd(int32_t dirs, int32_t B, int32_t T, int32_t H, const float* dy, const float* dh_n /* nullable */,
                 const float* wpack, const float* saved, size_t saved_floats, float* dgx, float* dgh,
                 float* dh0 /* nullable */, void* stream);
int seld_gru_kernel_label(int32_t op, int32_t H, char* buf, int32_t buflen);

#ifdef __cplusplus
}
#endif
#endif /* SELD_HIP_H */
