"""Case table of the quaternion transposed convolution (quaternion_ops.py:149-171 of the reference), shared by the
fixture generator (make_golden_tconv.py, runs against the reference) and the tests.  Pure data + closed-form inputs."""
import torch

from oracle.seld_oracle import closed_form_input

# x shape (input of the transposed conv), Cout, kernel, stride, padding, output_padding, dilation, bias
TCONV_CASES = [
    dict(name="t1d_k4_s2", x=(3, 8, 7), cout=8, k=(4,), stride=2, padding=1, output_padding=0, dilation=1, bias=True),
    dict(name="t1d_k3_s3_op1", x=(1, 4, 9), cout=8, k=(3,), stride=3, padding=2, output_padding=1, dilation=1, bias=False),
    dict(name="t1d_k3_s1_d3_op2", x=(3, 8, 11), cout=4, k=(3,), stride=1, padding=0, output_padding=2, dilation=3,
         bias=True),
    dict(name="t2d_k4_s2", x=(3, 8, 5, 7), cout=8, k=(4, 4), stride=2, padding=1, output_padding=0, dilation=1, bias=True),
    dict(name="t2d_k31_s21_op1", x=(1, 8, 6, 9), cout=12, k=(3, 1), stride=(2, 1), padding=(1, 0), output_padding=(1, 0),
         dilation=1, bias=True),
    dict(name="t2d_k1_s2_op1", x=(3, 4, 5, 5), cout=8, k=(1, 1), stride=2, padding=0, output_padding=1, dilation=1,
         bias=False),
    dict(name="t2d_k2_s2_d2", x=(1, 8, 7, 5), cout=8, k=(2, 2), stride=2, padding=2, output_padding=1, dilation=2,
         bias=True),
    dict(name="t2d_k3_s1", x=(3, 8, 6, 7), cout=8, k=(3, 3), stride=1, padding=1, output_padding=0, dilation=1,
         bias=False),
    dict(name="t2d_k3_s3_op2", x=(1, 4, 4, 5), cout=4, k=(3, 3), stride=3, padding=0, output_padding=2, dilation=1,
         bias=True),
]

# QuaternionTransposeConv with its own (seeded) initialisation: np.random.seed(LAYER_CASE["np_seed"]) first, as the
# quaternion initialiser draws from numpy's global generator
LAYER_CASE = dict(name="layer", x=(2, 8, 5, 6), in_channels=8, out_channels=12, kernel_size=3, stride=2, padding=1,
                  output_padding=1, dilatation=1, seed=5, np_seed=7)


def tconv_inputs(case, dtype=torch.float32):
    """Closed-form input, component weights (Cin/4, Cout/4, *k) and bias of a case."""
    x = closed_form_input(case["x"], dtype)
    wshape = (case["x"][1] // 4, case["cout"] // 4) + tuple(case["k"])
    numel = 1
    for s in wshape:
        numel *= s
    n = torch.arange(numel, dtype=torch.float64)
    ws = [(0.4 * torch.sin(0.37 * n + 1.3 * c + 0.2)).view(wshape).to(dtype) for c in range(4)]
    bias = None
    if case["bias"]:
        bias = (0.1 * torch.cos(torch.arange(case["cout"], dtype=torch.float64) * 0.9)).to(dtype)
    return x, ws, bias


def tconv_cotangent(y_shape, dtype=torch.float32):
    return closed_form_input(tuple(y_shape), dtype).flip(0) * 0.5 + 0.25
