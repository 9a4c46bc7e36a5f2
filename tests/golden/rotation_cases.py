"""Case table of the quaternion rotation ops (quaternion_conv_rotation, quaternion_transpose_conv_rotation,
quaternion_linear_rotation; quaternion_ops.py:174-388 of the reference), shared by the fixture generator
(make_golden_rotation.py, runs against the reference) and the tests.  Pure data, closed-form inputs and the rotation
weight restated from its formula (include/seld_hip.h)."""
import torch

from oracle.seld_oracle import closed_form_input

# kind: conv / tconv / linear.  w: component shape -- conv (O, I, *k), tconv (Iin, Oout, *k), linear (I, O).
# x: the input's shape with its channel (conv) or feature (linear) axis left out; it holds MB * I channels, MB = 3, or 4
# with quaternion_format.  Every case runs with both quaternion_format values, with and without bias (`variants`).
ROT_CASES = [
    dict(name="conv1d_k3_d2", kind="conv", x=(2, 13), w=(3, 2, 3), stride=1, padding=2, dilation=2),
    dict(name="conv2d_k3_s2", kind="conv", x=(2, 7, 9), w=(2, 3, 3, 3), stride=2, padding=1, dilation=1),
    dict(name="tconv1d_k4_s2", kind="tconv", x=(2, 7), w=(2, 3, 4), stride=2, padding=1, output_padding=0, dilation=1),
    dict(name="tconv2d_k3_s2_op1", kind="tconv", x=(1, 5, 6), w=(3, 2, 3, 3), stride=2, padding=1, output_padding=1,
         dilation=1),
    dict(name="linear2d", kind="linear", x=(5,), w=(3, 4)),
    dict(name="linear3d", kind="linear", x=(2, 3), w=(4, 2)),
]

# One seeded layer of each class in a configuration the reference can run (its layers' bias has 4*O elements, which only
# quaternion_format=True matches).  np.random.seed(np_seed) first: the quaternion initialiser draws from numpy's global
# generator.  x: the closed-form input of the layer.
LAYER_CASES = [
    dict(name="layer_conv", cls="QuaternionConv", x=(2, 8, 6, 7),
         kwargs=dict(in_channels=8, out_channels=12, kernel_size=3, stride=1, padding=1, bias=True,
                     rotation=True, quaternion_format=True, seed=5), np_seed=7),
    dict(name="layer_tconv", cls="QuaternionTransposeConv", x=(2, 8, 5, 6),
         kwargs=dict(in_channels=8, out_channels=12, kernel_size=3, stride=2, padding=1, output_padding=1, bias=True,
                     rotation=True, quaternion_format=True, seed=6), np_seed=8),
    dict(name="layer_linear", cls="QuaternionLinearAutograd", x=(3, 4, 12),
         kwargs=dict(in_features=16, out_features=8, bias=False, rotation=True, quaternion_format=False, seed=9),
         np_seed=9),
]


def variants(case):
    """(variant name, quaternion_format, bias) of a case."""
    return [(f"{case['name']}_q{int(q)}_b{int(b)}", q, b) for q in (False, True) for b in (False, True)]


def all_variants():
    return [(c, v, q, b) for c in ROT_CASES for v, q, b in variants(c)]


def mb(qformat):
    return 4 if qformat else 3


def out_channels(case, qformat):
    return mb(qformat) * (case["w"][0] if case["kind"] == "conv" else case["w"][1])


def rotation_inputs(case, qformat, bias, dtype=torch.float32):
    """Closed-form input, component weights and bias (None or out_channels elements) of a variant.  The weights keep
    |u| > 0.49 everywhere (the four phases span more than pi), away from the reference's n = 0 singularity."""
    w = case["w"]
    cin = mb(qformat) * (w[1] if case["kind"] == "conv" else w[0])
    if case["kind"] == "linear":
        xshape = tuple(case["x"]) + (cin,)
    else:
        xshape = (case["x"][0], cin) + tuple(case["x"][1:])
    x = closed_form_input(xshape, dtype)
    numel = 1
    for s in w:
        numel *= s
    n = torch.arange(numel, dtype=torch.float64)
    ws = [(0.4 * torch.sin(0.37 * n + 1.3 * c + 0.2)).view(w).to(dtype) for c in range(4)]
    b = None
    if bias:
        b = (0.1 * torch.cos(torch.arange(out_channels(case, qformat), dtype=torch.float64) * 0.9)).to(dtype)
    return x, ws, b


def rotation_cotangent(y_shape, dtype=torch.float32):
    return closed_form_input(tuple(y_shape), dtype).flip(0) * 0.5 + 0.25


def rotation_matrix(ws, qformat):
    """The real weight K (MB*A, MB*B, *taps) of component tensors (A, B, *taps), restated from the formula: per element
    n = |u|, f = 2n, E = I + f*Q(u); differentiable (autograd gives the reference's gradient)."""
    r, i, j, k = ws
    f = 2.0 * torch.sqrt(r * r + i * i + j * j + k * k)
    one = torch.ones_like(r)
    E = [[one - f * (j * j + k * k), f * (i * j + r * k), f * (i * k - r * j)],
         [f * (i * j - r * k), one - f * (i * i + k * k), f * (j * k + r * i)],
         [f * (i * k + r * j), f * (j * k - r * i), one - f * (i * i + j * j)]]
    if qformat:
        z = torch.zeros_like(r)
        E = [[z, z, z, z]] + [[z] + row for row in E]
    return torch.cat([torch.cat(row, dim=1) for row in E], dim=0)


def rotation_reference64(case, x, ws, bias, qformat):
    """The op of a case in torch on the host: K by rotation_matrix, then F.convNd / F.conv_transposeNd / x @ K + b."""
    import torch.nn.functional as F
    K = rotation_matrix(ws, qformat)
    if case["kind"] == "conv":
        fn = F.conv1d if x.dim() == 3 else F.conv2d
        return fn(x, K, bias, case["stride"], case["padding"], case["dilation"], 1)
    if case["kind"] == "tconv":
        fn = F.conv_transpose1d if x.dim() == 3 else F.conv_transpose2d
        return fn(x, K, bias, case["stride"], case["padding"], case["output_padding"], 1, case["dilation"])
    y = torch.matmul(x, K)
    return y + bias if bias is not None else y
