"""Writes tests/golden/hcq_dispatch.json: what the host-only queries of the fast-product ("hcq") convolution family answer
over the descriptor grid of make_golden_conv_dispatch.py plus the rows below -- packed-weight size, kernel label and launch
shape for mode 0 / 1 / 2 x npair 1 / 2, weight-gradient support and label, grouped weight-gradient family.  None of them
touches a device.

The fixture pins the dispatch (scheme and layout: make_golden_conv_dispatch.py, whose descriptors / encode / decode / dump
this module uses).  It was written by the library of the commit that precedes the one-table, one-plan launch code of
hcq_conv.hip and hcq_wgrad.hip.  That library had no seld_hcq_launch_shape: it was built with only that function added,
from a patch that is kept outside the tree.  The function reported the grid and LDS bytes of the launch (the pooling
kernel's LDS as hcq_first_pool_impl computed it), the rows per workgroup, and the ring offset and slot kind of launches
that HAVE a ring: for hcq_first_kernel, hcq_first_pool_kernel and the global-load form of hcq_conv_kernel, which never read
those two fields, it reported 0 and not what that library's plan happened to leave in them (it planned the ring before it
chose the first-layer kernel: 13824 or 6912 in 42 rows).  The one column that was regenerated afterwards is the label of
seld_hcq_wgrad_label, which lost its last template argument together with the kernel.  Re-run only when a dispatch change is
intended:

    python tests/golden/make_golden_hcq_dispatch.py

An answer has 12 fields: rc of seld_hc_conv_out_shape (a descriptor the library refuses has rc alone); per (mode, npair) in
the order of COMBOS one field [pack floats, [rc, label], [rc, grid x, grid y, LDS bytes, ring offset, half slots, first
rows]]; seld_hcq_wgrad_supported for npair 1 and 2; [rc, label] of seld_hcq_wgrad_label for npair 1 and 2;
seld_hcq_wgrad_group_family.
"""
import ctypes
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.golden import make_golden_conv_dispatch as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "hcq_dispatch.json")
COMBOS = tuple((mode, npair) for mode in (0, 1, 2) for npair in (1, 2))
NFIELDS = 1 + len(COMBOS) + 5

ENVS = [("default", {}), ("SELD_CONV_NO_HCQ=1", {"SELD_CONV_NO_HCQ": "1"}),
        ("SELD_CONV_NO_SMALLK=1", {"SELD_CONV_NO_SMALLK": "1"})]
SWITCHES = ("SELD_CONV_NO_HCQ", "SELD_CONV_NO_SMALLK")


def _c1(A, shape, cout, k, pad, dil):
    """A row from (algebra, x shape, cout, k, pad, dil) as the GPU tests write their cases."""
    n, cin = shape[0], shape[1]
    if len(shape) == 3:
        return A, cin, cout, (1, k), (1, 1), (1, dil), (0, pad), (1, shape[2]), n
    return A, cin, cout, tuple(k), (1, 1), (dil, dil), (pad, pad), tuple(shape[2:]), n


TCN_DILATIONS = (1, 2, 3, 5, 8, 13, 16, 21, 34, 55)

# Rows beyond the product grid: together they name every row of the instantiation table of hcq_conv.hip in every state
# the plan can produce (tests/test_hcq_dispatch_host.py lists them)
EXTRA = tuple(
    # HCQ_CASES of tests/test_gpu_conv.py
    [_c1(8, (2, 192, 128), 384, 3, 5, 5), _c1(8, (3, 192, 64), 384, 3, 55, 55), _c1(8, (2, 384, 128), 192, 1, 0, 1),
     _c1(8, (2, 192, 128), 128, 1, 0, 1), _c1(8, (1, 192, 4, 128), 192, (3, 3), 1, 1), _c1(8, (9, 192, 8, 512), 192, (3, 3), 1, 1),
     _c1(8, (2, 128, 3, 64), 128, (3, 3), 1, 1), _c1(4, (2, 64, 128), 128, 3, 2, 2), _c1(4, (2, 128, 64), 64, 1, 0, 1),
     _c1(4, (2, 64, 5, 64), 64, (3, 3), 1, 1), _c1(4, (3, 64, 192), 64, 3, 34, 34)] +
    # the first layers of test_hcq_forward_with_padded_k_groups
    [_c1(a, s, c, (3, 3), 1, 1) for a, s, c in (
        (8, (2, 8, 6, 128), 192), (8, (2, 16, 5, 64), 192), (4, (2, 8, 4, 64), 64), (8, (1, 48, 3, 64), 128),
        (4, (3, 12, 2, 128), 128), (8, (2, 8, 16, 128), 192), (8, (1, 16, 8, 192), 192), (8, (2, 8, 8, 64), 128),
        (4, (2, 8, 24, 64), 64), (4, (1, 4, 8, 128), 128))] +
    # ... the same with one tile in the dual quaternion and two in the quaternion at two block channels, and at the
    # benchmark's size (where the 8-channel layer is left to the short-K kernel unless SELD_CONV_NO_SMALLK is set)
    [_c1(8, (2, 16, 8, 64), 128, (3, 3), 1, 1), _c1(4, (1, 8, 8, 128), 128, (3, 3), 1, 1), _c1(4, (2, 4, 16, 64), 64, (3, 3), 1, 1),
     _c1(8, (32, 8, 128, 512), 192, (3, 3), 1, 1), _c1(8, (32, 16, 128, 512), 192, (3, 3), 1, 1)] +
    # the shapes of tests/test_gpu_hcq_fragment_ring.py that are not above
    [_c1(4, (1, 32, 64), 64, 1, 0, 1), _c1(4, (1, 192, 64), 64, 3, 1, 1), _c1(4, (1, 64, 3, 64), 64, (3, 3), 1, 1)] +
    # the TCN layers at W = 512, N = 32: dilated 1x3 192 -> 384 and its 1x1 384 -> 192, in both algebras
    [_c1(a, (32, 192, 512), 384, 3, d, d) for a in (8, 4) for d in TCN_DILATIONS] +
    [_c1(a, (32, 384, 512), 192, 1, 0, 1) for a in (8, 4)] +
    # few position tiles: the data gradient of 192 -> 384 keeps its mixed tile in workgroups of its own, with every halo
    [_c1(8, (2, 192, 128), 384, 3, d, d) for d in TCN_DILATIONS] +
    # ... and at N = 64 as three-tile workgroups (512 position tiles), with every halo
    [_c1(8, (64, 192, 512), 384, 3, d, d) for d in TCN_DILATIONS] +
    # 1x1 chunks of 24 and of 8 block channels in both algebras, one and two quaternion tiles; 1x3 chunk 4 in the
    # quaternion, in three-tile workgroups, and with a halo that leaves the two-tile launch no room for a ring
    [_c1(4, (2, 96, 128), 64, 1, 0, 1), _c1(4, (2, 96, 128), 128, 1, 0, 1), _c1(8, (2, 64, 128), 128, 1, 0, 1),
     _c1(4, (1, 32, 64), 128, 1, 0, 1), _c1(4, (2, 16, 128), 64, 3, 1, 1), _c1(4, (2, 48, 128), 128, 3, 1, 1),
     _c1(8, (2, 32, 128), 128, 3, 1, 1), _c1(8, (64, 96, 512), 192, 3, 1, 1), _c1(8, (2, 192, 128), 384, 3, 60, 60)]
)


def descriptors():
    yield from G.descriptors()
    yield from EXTRA


def _label(fn, *args):
    buf = ctypes.create_string_buffer(96)
    rc = fn(*args, buf, 96)
    return [rc, buf.value.decode() if rc == 0 else ""]


def answers(L, H, row):
    A, ci, co, k, s, d, p, hw, n = row
    lib = L.lib()
    desc = H.make_conv_desc((n, ci) + tuple(hw), co, A, k, s, p, d)
    ref = ctypes.byref(desc)
    out = (ctypes.c_int32 * 2)()
    rc = lib.seld_hc_conv_out_shape(ref, out)
    if rc != 0:
        return [rc]
    got = [rc]
    for mode, npair in COMBOS:
        shape = (ctypes.c_int32 * 6)()
        src = lib.seld_hcq_launch_shape(ref, mode, npair, shape)
        got.append([int(lib.seld_hcq_pack_floats(ref, mode, npair)), _label(lib.seld_hcq_kernel_label, ref, mode, npair),
                    [src] + (list(shape) if src == 0 else [])])
    got += [int(lib.seld_hcq_wgrad_supported(ref, npair)) for npair in (1, 2)]
    got += [_label(lib.seld_hcq_wgrad_label, ref, npair) for npair in (1, 2)]
    got.append(int(lib.seld_hcq_wgrad_group_family(ref)))
    return got


def walk(setenv):
    """{environment name: [answers(row) for every descriptor]} from the built library (see G.walk)."""
    P = importlib.import_module(G.PKG)
    L, H = P._lib, P.hip_ops
    rows = list(descriptors())
    got = {}
    for name, switches in ENVS:
        for sw in SWITCHES:
            setenv(sw, switches.get(sw))
        got[name] = [answers(L, H, row) for row in rows]
    for sw in SWITCHES:
        setenv(sw, None)
    return got


def encode(got):
    return G.encode(got, NFIELDS, G.BLOCK)


def decode(doc):
    return G.decode(doc, ENVS)


def main():
    L = importlib.import_module(G.PKG)._lib

    def setenv(name, value):
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value
        L.reload_env()
    got = walk(setenv)
    doc = encode(got)
    assert decode(doc) == got
    G.dump(doc, OUT)
    print(OUT, doc["rows"], "rows,", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
