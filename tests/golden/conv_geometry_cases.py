"""Case tables of the 1-D / 2-D hypercomplex convolution's geometry (stride, tap shapes, padding, dilation and the shapes
one step outside a fast kernel's gate), shared by the fixture generator (make_golden_conv_geometry.py, runs against the
reference) and the tests.  Pure data + input builders + the index arithmetic the tests reason with."""
import torch

from oracle.seld_oracle import closed_form_input


def _c(name, algebra, x, cout, k, stride=1, padding=0, dilation=1, bias=True, edge=False):
    return dict(name=name, algebra=algebra, x=x, cout=cout, k=k, stride=stride, padding=padding, dilation=dilation,
                bias=bias, edge=edge)


# Small: the reference's float64 results for all of them are the committed fixture.  Closed-form inputs.
FIXTURE_CASES = [
    # ---- dual quaternion, 1-D
    _c("dq1d_k3_s2_p1", 8, (2, 8, 19), 16, (3,), 2, 1),
    _c("dq1d_k5_s3_p2_d2", 8, (2, 16, 31), 8, (5,), 3, 2, 2),             # stride with dilation, 5 dilated taps
    _c("dq1d_k2_s3_tail", 8, (3, 8, 15), 8, (2,), 3, 0, bias=False),      # stride > extent: holes, and a trailing sample
    _c("dq1d_k1_s2_tail", 8, (2, 8, 10), 8, (1,), 2, 0),                  # k = 1, s = 2: every odd sample untouched
    _c("dq1d_k4_s2_p3", 8, (2, 8, 17), 8, (4,), 2, 3),
    _c("dq1d_k7_p5", 8, (1, 8, 12), 8, (7,), 1, 5),                       # p > (k - 1) / 2: output longer than the input
    # ---- dual quaternion, 2-D
    _c("dq2d_k33_s22_p1", 8, (2, 8, 7, 10), 8, (3, 3), (2, 2), 1),
    _c("dq2d_k31_s21_p10", 8, (1, 8, 9, 6), 16, (3, 1), (2, 1), (1, 0)),
    _c("dq2d_k15_s12_p02", 8, (2, 8, 4, 13), 8, (1, 5), (1, 2), (0, 2)),
    _c("dq2d_k55_s32_p2", 8, (1, 8, 12, 11), 8, (5, 5), (3, 2), 2, bias=False),
    _c("dq2d_k23_s22_tail", 8, (2, 8, 9, 10), 8, (2, 3), (2, 2), 0),      # a trailing row and a trailing column untouched
    _c("dq2d_k33_d23_p34", 8, (1, 8, 6, 9), 8, (3, 3), 1, (3, 4), (2, 3)),   # dilation (2, 3), output larger than the input
    _c("dq2d_k12_p23", 8, (2, 8, 3, 5), 8, (1, 2), 1, (2, 3)),            # padding >= the kernel extent on both axes
    _c("dq2d_k33_p0", 8, (1, 16, 5, 8), 8, (3, 3), 1, 0),                 # valid 3x3
    # ---- quaternion
    _c("q1d_k5_s2_p2", 4, (2, 8, 18), 12, (5,), 2, 2),
    _c("q2d_k55_s21_p20", 4, (1, 4, 9, 8), 8, (5, 5), (2, 1), (2, 0)),
    # ---- real
    _c("r1d_k7_s2_p4", 1, (2, 3, 23), 5, (7,), 2, 4),
    _c("r2d_k23_s12_p03", 1, (2, 3, 6, 7), 4, (2, 3), (1, 2), (0, 3)),
]

# Medium: shapes that reach the FAST forward template, the 32-position and the row-chunk weight gradients, and the
# benchmark's layers (192 / 384 channels, 3x3 or 1x3 'same') with ONE property moved just outside a fast kernel's gate
# (edge=True).  Seeded random inputs; compared with the float64 oracle only.
_MEDIUM_CASES = [
    _c("dq1d_fast_s2", 8, (2, 64, 256), 64, (3,), 2, 1),                  # Cin/8 * 3 = 24: FAST forward with SMw = 2
    _c("dq2d_fast_row_s21", 8, (2, 32, 9, 64), 32, (3, 3), (2, 1), 1),    # FAST forward with SMh = 2; row wgrad, sh = 2
    _c("dq2d_row_p0", 8, (2, 16, 6, 66), 16, (3, 3), 1, 0),               # row wgrad, ph = pw = 0 (66 -> 64 columns)
    _c("dq2d_row_dh2", 8, (1, 128, 6, 64), 128, (3, 3), 1, (2, 1), (2, 1)),   # hcq-eligible but for dil_h = 2; row wgrad
    _c("dq2d_w32_s21", 8, (2, 16, 9, 36), 16, (3, 3), (2, 1), 1),         # 36 columns: hc_wgrad32_kernel with sh = 2
    _c("dq2d_k33_s12_p1", 8, (2, 16, 6, 40), 16, (3, 3), (1, 2), 1),      # stride along W only
    _c("dq1d_k7_s2_p3", 8, (2, 16, 100), 24, (7,), 2, 3),
    _c("q2d_k31_s21_w32", 4, (2, 16, 10, 32), 16, (3, 1), (2, 1), (1, 0)),        # generic taps on hc_wgrad32_kernel
    _c("r2d_k33_s22_p1", 1, (2, 6, 11, 37), 10, (3, 3), (2, 2), 1),
    # ---- gate edges
    _c("edge_w520", 8, (1, 192, 520), 384, (3,), 1, 1, edge=True),        # W % 64 != 0; outW % 4 == 0, % 32 != 0
    _c("edge_w72_3x3", 8, (1, 192, 2, 72), 192, (3, 3), 1, 1, edge=True),
    _c("edge_odd_w", 8, (1, 192, 65), 384, (3,), 1, 1, edge=True),        # odd outW: the 16-position weight gradient
    _c("edge_w24", 8, (2, 192, 24), 384, (3,), 1, 1, edge=True),          # outW < 32
    _c("edge_short_k", 8, (2, 8, 64), 192, (3,), 1, 1, edge=True),        # Cin/8 * 3 = 3: < 16 and not a multiple of 4
    _c("edge_cout40", 8, (2, 192, 64), 40, (3,), 1, 1, edge=True),        # 5 block channels: fills no tile
    _c("edge_h1", 8, (2, 192, 1, 72), 192, (1, 3), 1, (0, 1), edge=True),   # 2-D input with H = 1
]

GPU_CASES = FIXTURE_CASES + _MEDIUM_CASES


# ---- geometry ---------------------------------------------------------------------------------------------------------
def geometry(case):
    """Per spatial axis: input extent, kernel, stride, padding, dilation (tuples of the input's spatial rank)."""
    nd = len(case["x"]) - 2

    def per_axis(v):
        return (int(v),) * nd if isinstance(v, int) else tuple(int(e) for e in v)
    return dict(nd=nd, inp=tuple(case["x"][2:]), k=tuple(case["k"]), s=per_axis(case["stride"]),
                p=per_axis(case["padding"]), d=per_axis(case["dilation"]))


def span(g, a):
    """in + 2p - d(k - 1) - 1 of axis a: the last admissible start of the kernel in the padded input."""
    return g["inp"][a] + 2 * g["p"][a] - g["d"][a] * (g["k"][a] - 1) - 1


def out_extent(case):
    g = geometry(case)
    return tuple(span(g, a) // g["s"][a] + 1 for a in range(g["nd"]))


def remainder(case):
    g = geometry(case)
    return tuple(span(g, a) % g["s"][a] for a in range(g["nd"]))


def touched(case):
    """Per axis, which input samples any (output position, tap) reads: list of lists of bool."""
    g = geometry(case)
    out = out_extent(case)
    masks = []
    for a in range(g["nd"]):
        m = [False] * g["inp"][a]
        for o in range(out[a]):
            for t in range(g["k"][a]):
                i = o * g["s"][a] + t * g["d"][a] - g["p"][a]
                if 0 <= i < g["inp"][a]:
                    m[i] = True
        masks.append(m)
    return masks


def untouched_mask(case):
    """Bool tensor over the spatial axes of x: True where no output reads the sample, so dx is exactly 0.0 there."""
    masks = [~torch.tensor(m) for m in touched(case)]
    if len(masks) == 1:
        return masks[0]
    return masks[0][:, None] | masks[1][None, :]


def weight_shape(case):
    A = case["algebra"]
    return (case["cout"] // A, case["x"][1] // A) + tuple(case["k"])


# ---- inputs -----------------------------------------------------------------------------------------------------------
def fixture_inputs(case, dtype=torch.float32):
    """Closed-form input, component weights and bias of a case."""
    x = closed_form_input(case["x"], dtype)
    wshape = weight_shape(case)
    numel = 1
    for s in wshape:
        numel *= s
    n = torch.arange(numel, dtype=torch.float64)
    ws = [(0.4 * torch.sin(0.37 * n + 1.3 * c + 0.2)).view(wshape).to(dtype) for c in range(case["algebra"])]
    bias = None
    if case["bias"]:
        bias = (0.1 * torch.cos(torch.arange(case["cout"], dtype=torch.float64) * 0.9)).to(dtype)
    return x, ws, bias


def fixture_cotangent(y_shape, dtype=torch.float32):
    return closed_form_input(tuple(y_shape), dtype).flip(0) * 0.5 + 0.25


def random_inputs(case, seed=1234):
    """Seeded float32 x, component weights (x 0.2), bias and cotangent of a case."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(case["x"], generator=gen)
    ws = [torch.randn(weight_shape(case), generator=gen) * 0.2 for _ in range(case["algebra"])]
    bias = torch.randn(case["cout"], generator=gen) if case["bias"] else None
    y_shape = (case["x"][0], case["cout"]) + out_extent(case)
    cot = torch.randn(y_shape, generator=gen)
    return x, ws, bias, cot
