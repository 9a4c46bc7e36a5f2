"""Launches that pin the bits of the stride-phase / forward implicit GEMM (csrc/hc_phase_gemm.h) behind
hc_tconv_kernel, hc_conv3d_fwd_kernel and hc_conv3d_phase_kernel.  Shared by tests/test_gpu_phase_gemm.py and
tests/golden/make_golden_phase_gemm.py, which writes phase_gemm_bits.json from the library that precedes a change to
that body.

Inputs are seeded torch.randn floats (weights times 0.1, as tools/tconv_bench.py draws them), never integers: a
changed summation order has to show in the bits.

TWIN_CASES: 2-D (or 1-D) transposed convolutions.  Each also runs lifted to depth 1 through the 3-D transposed
forward, which must give the same bits.  Case 9 has 44352 output channels: the tile choice takes <12, 1> only once
both it and <4, 4> fill the device, and at this case's 128 output positions that needs 231 channel tiles of 192 (with
the 192 channels first tried the plan took <1, 4>).

C3_CASES: true 3-D launches.  `op`: conv3d forward ("fwd"), its input gradient ("dgrad"), or the transposed forward
("tfwd").
"""
import hashlib

import torch


def _t(name, algebra, x, cout, k, stride, padding, output_padding, dilation, bias, what):
    return dict(name=name, algebra=algebra, x=x, cout=cout, k=k, stride=stride, padding=padding,
                output_padding=output_padding, dilation=dilation, bias=bias, what=what)


TWIN_CASES = [
    _t("s2_k4", 4, (2, 8, 5, 12), 8, (4, 4), 2, 1, 0, 1, True, "sw > 1 scalar stores, Qw % 4 == 0"),
    _t("s1_k3_tails", 4, (3, 20, 6, 16), 20, (3, 3), 1, 1, 0, 1, True, "sw == 1 vector stores, channel tails on both sides"),
    _t("real_s3_op2", 1, (2, 7, 5, 7), 5, (2, 2), 3, 0, (2, 2), 1, True,
       "classes no tap reaches, which get the bias alone; Qw % 4 != 0"),
    _t("s2_d2", 4, (1, 4, 6, 9), 12, (3, 3), 2, 2, 1, 2, False, "gcd(stride, dilation) > 1"),
    _t("s1_d3_op2", 4, (2, 4, 5, 6), 4, (2, 3), 1, 0, 2, 3, True, "output padding >= stride, legal because < dilation"),
    _t("s21", 4, (2, 8, 4, 16), 8, (4, 3), (2, 1), (1, 1), 0, 1, True, "mixed strides"),
    _t("one_d", 4, (2, 8, 19), 8, (4,), 2, 1, 0, 1, True, "the 1-D form"),
    _t("tile_spans_images", 4, (9, 4, 3, 5), 4, (1, 1), 1, 0, 0, 1, False, "one 256-position tile spans every image"),
    _t("tile_12x1", 4, (1, 16, 4, 8), 44352, (3, 3), 2, 1, 1, 1, True, "tile <12, 1>"),
    _t("tile_4x4", 4, (1, 4, 384, 128), 64, (1, 1), 1, 0, 0, 1, True,
       "tile <4, 4>: q_t1x1_c4_o64_n1_384x128 of hc_exact_cases.py"),
]
# the three tiles the 2-D plan can reach (tests/test_hc_exact_host.py)
TWIN_TILES = {"hc_tconv_kernel<12, 1>", "hc_tconv_kernel<4, 4>", "hc_tconv_kernel<1, 4>"}


def _c(name, op, algebra, x, cout, k, stride, padding, label, what):
    return dict(name=name, op=op, algebra=algebra, x=x, cout=cout, k=k, stride=stride, padding=padding, label=label,
                what=what)


_DQ = dict(algebra=8, x=(1, 32, 2, 4, 8), cout=32, k=(1, 3, 3), stride=(1, 2, 2), padding=(0, 1, 1))
C3_CASES = [
    _c("q_fwd_s121", "fwd", 4, (2, 8, 3, 5, 6), 8, (3, 3, 3), (1, 2, 1), 1, None, "quaternion forward, mixed strides"),
    dict(_DQ, name="dq_fwd_halves", op="fwd", label="hc_conv3d_fwd_kernel<1, 4>",
         what="16-channel tiles, each wholly in one half: zero-quadrant skip of the forward map"),
    dict(_DQ, name="dq_dgrad_halves", op="dgrad", label="hc_conv3d_phase_kernel<1, 4>",
         what="the same skip with the weights read transposed"),
    _c("q_tfwd_s2", "tfwd", 4, (1, 8, 2, 3, 5), 8, (2, 2, 2), 2, 0, None, "quaternion transposed forward"),
    _c("q_fwd_tile_4x1", "fwd", 4, (6, 8, 4, 8, 8), 64, (3, 3, 3), 2, 1, "hc_conv3d_fwd_kernel<4, 1>",
       "the 3-D-only tile: 64 channels x 192 positions"),
]


def _seed(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


def _draw(case, w_shape, y_shape=None):
    """x, the component tensors, the bias (or None) and, for y_shape, a cotangent: CPU float32, seeded by the name."""
    gen = torch.Generator().manual_seed(_seed(case["name"]))
    x = torch.randn(case["x"], generator=gen)
    ws = [torch.randn(w_shape, generator=gen) * 0.1 for _ in range(case["algebra"])]
    bias = torch.randn(case["cout"], generator=gen) if case.get("bias", True) else None
    dy = torch.randn(y_shape, generator=gen) if y_shape else None
    return x, ws, bias, dy


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _lift(v, fill, nd):
    """A 1-D or 2-D geometry value (int or nd-tuple) on (D, H, W), `fill` on the new leading axes."""
    v = tuple(v) if isinstance(v, (tuple, list)) else (v,) * nd
    return (fill,) * (3 - len(v)) + v


def run_twin(H, case, dev):
    """(label, y of the 2-D transposed forward, y of the same problem at depth 1 on the 3-D transposed forward)."""
    A, cin, cout = case["algebra"], case["x"][1], case["cout"]
    x, ws, bias, _ = _draw(case, (cin // A, cout // A) + tuple(case["k"]))
    x, ws = x.to(dev), [w.to(dev) for w in ws]
    bias = bias.to(dev) if bias is not None else None
    desc, op = H.conv_transpose_desc(case["x"], cout, A, case["k"], case["stride"], case["padding"],
                                     case["output_padding"], case["dilation"])
    label = H.conv_transpose_label(desc, op, 0)
    y2 = H.conv_transpose_fwd(desc, op, x, ws, bias)
    nd = len(case["x"]) - 2
    x3, w3 = x, ws
    for _ in range(3 - nd):
        x3, w3 = x3.unsqueeze(2), [w.unsqueeze(2) for w in w3]
    geo = [_lift(case[f], fill, nd) for f, fill in (("k", 1), ("stride", 1), ("padding", 0), ("output_padding", 0),
                                                    ("dilation", 1))]
    d3, op3 = H.conv3d_transpose_desc(tuple(x3.shape), cout, A, *geo)
    y3 = H.conv3d_fwd(d3, op3, x3, w3, bias)
    return label, y2, y3


def run_c3(H, case, dev):
    """(label, result) of one 3-D launch."""
    A, cin, cout, op = case["algebra"], case["x"][1], case["cout"], case["op"]
    if op == "tfwd":
        desc, out_pad = H.conv3d_transpose_desc(case["x"], cout, A, case["k"], case["stride"], case["padding"], 0, 1)
        w_shape = (cin // A, cout // A) + tuple(case["k"])
    else:
        desc, out_pad = H.make_conv3d_desc(case["x"], cout, A, case["k"], case["stride"], case["padding"], 1), None
        w_shape = (cout // A, cin // A) + tuple(case["k"])
    y_shape = (case["x"][0], cout) + H.conv3d_out_shape(desc, out_pad)
    x, ws, bias, dy = _draw(case, w_shape, y_shape if op == "dgrad" else None)
    ws = [w.to(dev) for w in ws]
    if op == "dgrad":
        return H.conv3d_label(desc, None, 1), H.conv3d_bwd_data(desc, None, dy.to(dev), ws, tuple(case["x"]))
    return H.conv3d_label(desc, out_pad, 0), H.conv3d_fwd(desc, out_pad, x.to(dev), ws, bias.to(dev))
