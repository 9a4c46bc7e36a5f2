"""Cases of tests/golden/quat_algebra.npz: the element-wise quaternion algebra of the reference's quaternion_ops.py
(module "Q": get_modulus, get_normalized, hamilton_product) and dual_quaternion_ops.py (module "D": those three,
q_normalize and quaternion_exp).  Shared by make_golden_quat_algebra.py (runs the reference) and the tests.  Pure data
and closed-form inputs (no RNG).

A case names the module, the function, the input shape and the keyword arguments.  The list covers every rank each
module accepts and every rank it refuses (the generator records which cases the reference raises on, and how), both
modulus forms, a last-axis extent M that is and is not a multiple of 4, odd Q, outer = 1, a component axis that 4 does
not divide, and dim 0 long enough that the sum over it is split into more than one partial."""
import math

import torch

S2, S2V, S3, S4, S4V, S5 = (7, 20), (6, 16), (3, 5, 12), (2, 8, 3, 5), (2, 12, 4, 6), (2, 4, 2, 3, 4)
LONG2, LONG3 = (2100, 4), (600, 2, 8)


def _c(name, module, op, shape, **kwargs):
    return dict(name=name, module=module, op=op, shape=shape, kwargs=kwargs)


QUAT_ALGEBRA_CASES = [
    # ---- quaternion_ops: rank 2 and 3 only
    _c("q_modv_2d", "Q", "get_modulus", S2, vector_form=True),
    _c("q_mods_2d", "Q", "get_modulus", S2),
    _c("q_mods_2d_m4", "Q", "get_modulus", S2V, vector_form=False),
    _c("q_mods_2d_long", "Q", "get_modulus", LONG2),
    _c("q_modv_3d", "Q", "get_modulus", S3, vector_form=True),
    _c("q_mods_3d", "Q", "get_modulus", S3),
    _c("q_norm_2d", "Q", "get_normalized", S2),
    _c("q_norm_2d_eps", "Q", "get_normalized", S2V, eps=0.01),
    _c("q_norm_3d", "Q", "get_normalized", S3),
    _c("q_norm_3d_long", "Q", "get_normalized", LONG3),
    _c("q_ham_2d", "Q", "hamilton_product", S2),
    _c("q_ham_2d_m4", "Q", "hamilton_product", S2V),
    _c("q_ham_2d_outer1", "Q", "hamilton_product", (1, 12)),
    _c("q_ham_3d", "Q", "hamilton_product", S3),
    _c("q_modv_4d", "Q", "get_modulus", S4, vector_form=True),
    _c("q_mods_5d", "Q", "get_modulus", S5),
    _c("q_norm_4d", "Q", "get_normalized", S4),
    _c("q_ham_4d", "Q", "hamilton_product", S4),
    _c("q_mods_2d_bad", "Q", "get_modulus", (4, 10)),
    _c("q_norm_3d_bad", "Q", "get_normalized", (2, 3, 6)),
    _c("q_ham_2d_bad", "Q", "hamilton_product", (4, 10)),
    # ---- dual_quaternion_ops: rank 2 to 5
    _c("d_modv_2d", "D", "get_modulus", S2, vector_form=True),
    _c("d_mods_2d", "D", "get_modulus", S2),
    _c("d_mods_2d_long", "D", "get_modulus", LONG2),
    _c("d_norm_2d", "D", "get_normalized", S2),
    _c("d_norm_2d_long", "D", "get_normalized", LONG2, eps=0.001),
    _c("d_unit_2d", "D", "q_normalize", S2),
    _c("d_unit_2d_m4", "D", "q_normalize", S2V, channel=1),
    _c("d_unit_2d_ch0", "D", "q_normalize", S2, channel=0),
    _c("d_unit_2d_chm1", "D", "q_normalize", S2, channel=-1),
    _c("d_exp_2d", "D", "quaternion_exp", S2),
    _c("d_exp_2d_m4", "D", "quaternion_exp", S2V),
    _c("d_ham_2d", "D", "hamilton_product", S2),
    _c("d_modv_3d", "D", "get_modulus", S3, vector_form=True),
    _c("d_mods_3d", "D", "get_modulus", S3),
    _c("d_mods_3d_long", "D", "get_modulus", LONG3),
    _c("d_norm_3d", "D", "get_normalized", S3),
    _c("d_unit_3d", "D", "q_normalize", S3),
    _c("d_unit_3d_m4", "D", "q_normalize", (2, 3, 16)),
    _c("d_unit_3d_ch2", "D", "q_normalize", S3, channel=2),
    _c("d_unit_3d_ch0", "D", "q_normalize", S3, channel=0),
    _c("d_exp_3d", "D", "quaternion_exp", S3),
    _c("d_exp_3d_m4", "D", "quaternion_exp", (2, 3, 16)),
    _c("d_ham_3d", "D", "hamilton_product", S3),
    _c("d_modv_4d", "D", "get_modulus", S4, vector_form=True),
    _c("d_mods_4d", "D", "get_modulus", S4),
    _c("d_mods_4d_m4", "D", "get_modulus", S4V),
    _c("d_norm_4d", "D", "get_normalized", S4),
    _c("d_unit_4d", "D", "q_normalize", S4),
    _c("d_unit_4d_m4", "D", "q_normalize", S4V),
    _c("d_unit_4d_ch3", "D", "q_normalize", S4, channel=3),
    _c("d_exp_4d", "D", "quaternion_exp", S4),
    _c("d_exp_4d_outer1", "D", "quaternion_exp", (1, 8, 2, 6)),
    _c("d_ham_4d", "D", "hamilton_product", S4),
    _c("d_ham_4d_m4", "D", "hamilton_product", S4V),
    _c("d_modv_5d", "D", "get_modulus", S5, vector_form=True),
    _c("d_mods_5d", "D", "get_modulus", S5),
    _c("d_norm_5d", "D", "get_normalized", S5),
    _c("d_unit_5d", "D", "q_normalize", S5),
    _c("d_exp_5d", "D", "quaternion_exp", S5),
    _c("d_ham_5d", "D", "hamilton_product", S5),
    _c("d_unit_2d_bad", "D", "q_normalize", (4, 10)),
    _c("d_mods_4d_bad", "D", "get_modulus", (2, 6, 3, 3)),
    _c("d_exp_3d_bad", "D", "quaternion_exp", (2, 3, 6)),
]
CASE_IDS = [c["name"] for c in QUAT_ALGEBRA_CASES]


def closed_form(shape, phase, dtype=torch.float32):
    """sin(0.37 n + phase) + 0.5 cos((0.011 n^2) mod 2 pi + phase) over the flat index n, evaluated in float64: values in
    [-1.5, 1.5] with no period the shapes could lock onto, and some quaternions close to zero in every case."""
    n = torch.arange(math.prod(shape), dtype=torch.float64)
    v = torch.sin(0.37 * n + phase) + 0.5 * torch.cos(torch.remainder(0.011 * n * n, 2.0 * math.pi) + phase)
    return v.view(shape).to(dtype)


def _phase(case, k):
    return 0.1 + 0.61 * CASE_IDS.index(case["name"]) + 1.3 * k


def _envelope(shape, phase):
    """0.02 + 0.98 sin^2(1.7 k + phase) over the quaternion index k, shaped to multiply the four components of
    quaternion k alike: whole quaternions shrink towards zero (down to 0.02 of their size), which is where the three
    regularisations (1e-4 inside the root, outside it, eps on the summed root) differ.  None when 4 does not divide the
    component axis."""
    axis = len(shape) - 1 if len(shape) < 4 else 1
    if shape[axis] % 4:
        return None
    small = list(shape)
    small[axis] //= 4
    k = torch.arange(math.prod(small), dtype=torch.float64).view(small)
    return torch.cat([0.02 + 0.98 * torch.sin(1.7 * k + phase) ** 2] * 4, axis)


def quat_inputs(case, dtype=torch.float32):
    """The case's positional arguments: (input,) or (q0, q1), evaluated in float64."""
    out = []
    for k in range(2 if case["op"] == "hamilton_product" else 1):
        x = closed_form(case["shape"], _phase(case, k), torch.float64)
        env = _envelope(case["shape"], _phase(case, k))
        out.append((x if env is None else x * env).to(dtype))
    return tuple(out)


def quat_cotangent(case, y_shape, dtype=torch.float32):
    return closed_form(tuple(y_shape), _phase(case, 2), dtype)
