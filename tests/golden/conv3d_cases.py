"""Case table of the 3-D convolutions (F.conv3d / F.conv_transpose3d in quaternion_conv, dual_quaternion_conv,
quaternion_transpose_conv and the rotation variants; quaternion_ops.py:125-295, dual_quaternion_ops.py:111-153 of the
reference), shared by the fixture generator (make_golden_conv3d.py, runs against the reference) and the tests.  Pure
data + closed-form inputs."""
import torch

from oracle.seld_oracle import closed_form_input

# kind: conv (algebra 4 or 8) or tconv (algebra 4).  x: input shape (N, C, D, H, W); cout: output channels.
CONV3D_CASES = [
    dict(name="q_k3_same", kind="conv", algebra=4, x=(1, 8, 5, 6, 7), cout=8, k=(3, 3, 3), stride=1, padding=1,
         dilation=1, bias=True),
    dict(name="q_k133_odd", kind="conv", algebra=4, x=(1, 4, 3, 5, 7), cout=8, k=(1, 3, 3), stride=1, padding=(0, 1, 1),
         dilation=1, bias=False),
    dict(name="q_s121_d211", kind="conv", algebra=4, x=(1, 8, 5, 9, 7), cout=4, k=(3, 3, 3), stride=(1, 2, 1),
         padding=(2, 1, 1), dilation=(2, 1, 1), bias=True),
    dict(name="q_k233_s2", kind="conv", algebra=4, x=(1, 4, 7, 5, 9), cout=4, k=(2, 3, 3), stride=2, padding=0,
         dilation=1, bias=False),
    dict(name="dq_k3_same", kind="conv", algebra=8, x=(1, 8, 4, 5, 6), cout=16, k=(3, 3, 3), stride=1, padding=1,
         dilation=1, bias=True),
    dict(name="dq_k313_s212", kind="conv", algebra=8, x=(1, 16, 5, 7, 6), cout=8, k=(3, 1, 3), stride=(2, 1, 2),
         padding=(1, 0, 1), dilation=1, bias=False),
    dict(name="t_k3_s221_op100", kind="tconv", algebra=4, x=(2, 8, 3, 4, 5), cout=8, k=(3, 3, 3), stride=(2, 2, 1),
         padding=1, output_padding=(1, 0, 0), dilation=1, bias=True),
    dict(name="t_k232_s123_op012", kind="tconv", algebra=4, x=(1, 4, 3, 3, 4), cout=8, k=(2, 3, 2), stride=(1, 2, 3),
         padding=(0, 1, 0), output_padding=(0, 1, 2), dilation=1, bias=False),
]

# rotation ops: w the component shape, conv (O, I, *k), tconv (Iin, Oout, *k); x the input shape without its channel
# axis (MB * I channels, MB = 4 with quaternion_format, else 3).  Both quaternion_format values, with bias.
ROT3D_CASES = [
    dict(name="rot_conv_k3", kind="conv", x=(1, 4, 5, 6), w=(2, 2, 3, 3, 3), stride=1, padding=1, dilation=1),
    dict(name="rot_tconv_k233_s212", kind="tconv", x=(1, 3, 4, 3), w=(2, 2, 2, 3, 3), stride=(2, 1, 2),
         padding=(0, 1, 1), output_padding=(1, 0, 0), dilation=1),
]

# seeded layers with operation='convolution3d'.  np.random.seed(np_seed) first: the quaternion initialiser draws from
# numpy's global generator.  The rotation layer uses quaternion_format=True, the only setting its 4*O bias matches.
LAYER3D_CASES = [
    dict(name="layer_qconv", cls="QuaternionConv", x=(1, 8, 4, 5, 6),
         kwargs=dict(in_channels=8, out_channels=12, kernel_size=3, stride=1, padding=1, seed=5,
                     operation='convolution3d'), np_seed=7),
    dict(name="layer_dqconv", cls="DualQuaternionConv", x=(1, 16, 4, 5, 6),
         kwargs=dict(in_channels=16, out_channels=8, kernel_size=(1, 3, 3), stride=(1, 2, 1), padding=(0, 1, 1), seed=6,
                     operation='convolution3d'), np_seed=8),
    dict(name="layer_qtconv", cls="QuaternionTransposeConv", x=(2, 8, 3, 4, 4),
         kwargs=dict(in_channels=8, out_channels=4, kernel_size=3, stride=2, padding=1, output_padding=1, seed=9,
                     operation='convolution3d'), np_seed=9),
    dict(name="layer_qconv_rot", cls="QuaternionConv", x=(1, 8, 4, 4, 5),
         kwargs=dict(in_channels=8, out_channels=8, kernel_size=3, stride=1, padding=1, seed=11,
                     operation='convolution3d', rotation=True, quaternion_format=True), np_seed=10),
]


def conv3d_inputs(case, dtype=torch.float32):
    """Closed-form input, component weights -- conv (Cout/A, Cin/A, *k), tconv (Cin/A, Cout/A, *k) -- and bias."""
    A = case["algebra"]
    x = closed_form_input(case["x"], dtype)
    cin, cout = case["x"][1], case["cout"]
    wshape = ((cout // A, cin // A) if case["kind"] == "conv" else (cin // A, cout // A)) + tuple(case["k"])
    ws = _weights(wshape, A, dtype)
    bias = None
    if case["bias"]:
        bias = (0.1 * torch.cos(torch.arange(cout, dtype=torch.float64) * 0.9)).to(dtype)
    return x, ws, bias


def _weights(wshape, n, dtype):
    numel = 1
    for s in wshape:
        numel *= s
    i = torch.arange(numel, dtype=torch.float64)
    return [(0.4 * torch.sin(0.37 * i + 1.3 * c + 0.2)).view(wshape).to(dtype) for c in range(n)]


def rot3d_variants():
    """(case, variant name, quaternion_format) of every rotation case."""
    return [(c, f"{c['name']}_q{int(q)}", q) for c in ROT3D_CASES for q in (False, True)]


def rot3d_inputs(case, qformat, dtype=torch.float32):
    """Closed-form input, the four component tensors and a bias of the op's output channels."""
    m = 4 if qformat else 3
    w = case["w"]
    cin = m * (w[1] if case["kind"] == "conv" else w[0])
    cout = m * (w[0] if case["kind"] == "conv" else w[1])
    x = closed_form_input((case["x"][0], cin) + tuple(case["x"][1:]), dtype)
    ws = _weights(w, 4, dtype)
    bias = (0.1 * torch.cos(torch.arange(cout, dtype=torch.float64) * 0.9)).to(dtype)
    return x, ws, bias


def conv3d_cotangent(y_shape, dtype=torch.float32):
    return closed_form_input(tuple(y_shape), dtype).flip(0) * 0.5 + 0.25
