"""Case table of the depthwise-separable layers (DepthwiseSeparableConv2D / DepthwiseSeparableConv1D,
dual_quaternion_layers.py:19-47 of the reference), shared by the fixture generator (make_golden_depthwise.py, runs against
the reference) and the tests.  Pure data + closed-form inputs."""
import torch

from oracle.seld_oracle import closed_form_input

# cls: 2D or 1D; args: the constructor's (in_channels, out_channels, kernel_size, stride, padding); seed: the
# torch.manual_seed the layer is built under (its default initialisation draws from torch's generator); x: input shape.
DEPTHWISE_CASES = [
    dict(name="d2_k3_s1_p1", cls="2D", args=(4, 6, 3, 1, 1), seed=3, x=(2, 4, 7, 9)),
    dict(name="d2_k5_s2_p0", cls="2D", args=(3, 5, 5, 2, 0), seed=4, x=(2, 3, 11, 13)),
    dict(name="d2_k35_s1_p12", cls="2D", args=(4, 4, (3, 5), 1, (1, 2)), seed=5, x=(2, 4, 8, 10)),
    dict(name="d2_k3_s2_p1", cls="2D", args=(5, 8, 3, 2, 1), seed=6, x=(3, 5, 9, 12)),
    dict(name="d1_k3_s1_p0", cls="1D", args=(6, 4, 3, 1, 0), seed=7, x=(2, 6, 17)),
    dict(name="d1_k5_s2_p2", cls="1D", args=(4, 8, 5, 2, 2), seed=8, x=(3, 4, 23)),
    dict(name="d1_k5_s1_p2", cls="1D", args=(3, 5, 5, 1, 2), seed=9, x=(2, 3, 16)),
]

# parameter and buffer names, in state-dict order (those of torch.nn.Conv / BatchNorm under the reference's names)
PARAMS = ["depthwise.weight", "depthwise.bias", "pointwise.weight", "pointwise.bias", "bn.weight", "bn.bias"]
STATS = ["bn.running_mean", "bn.running_var", "bn.num_batches_tracked"]


def depthwise_input(case, dtype=torch.float32):
    return closed_form_input(case["x"], dtype)


def depthwise_cotangent(y_shape, dtype=torch.float32):
    return closed_form_input(tuple(y_shape), dtype).flip(0) * 0.5 + 0.25
