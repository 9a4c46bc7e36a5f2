"""Launches that pin the bits of the forward / data-gradient block-matrix kernels: hc_conv_kernel (csrc/hc_conv_fwd.hip),
hc_conv_vec_kernel (hc_conv_vec.hip) and hc_conv_smallk_kernel (hc_conv_smallk.hip), and of what they share
(csrc/hc_conv_tile.h: tile origin, K range, epilogue, statistics flush).  Shared by tests/test_gpu_hc_conv_bits.py and
tests/golden/make_golden_hc_conv_bits.py, which writes hc_conv_bits.json from the library that precedes a change to them.

The exact tests (test_gpu_hc_exact.py) feed small integers, exact in any summation order: they cannot see a reordered
float addition in the epilogue (bias, addend, old value, the s1 / s2 partial sums, the fold over lanes and waves).  Here
the inputs are the seeded randn draw of tests/hc_exact.py, so a changed order shows in the bits.

NAMES takes cases from tests/golden/hc_exact_cases.py, so labels and environments are pinned there.  traits() derives
from a case's labels and shape what the launch exercises; REQUIRED lists what the chosen cases must cover between them,
asserted below.

Statistics are summed with float atomics into row blockIdx.x % STATS_REPLICAS of the replica table, so they are
bit-stable only where a row receives ONE workgroup's contribution per channel: at most STATS_REPLICAS position tiles.
digests_stats() is that condition; larger launches, and every small-K one (it needs 32768 positions, its persistent
workgroups share rows), digest y alone -- their statistics stay held by the exact tests."""
import ctypes
import hashlib
import re

import torch

from tests import hc_exact as X

STATS_REPLICAS = 64           # SELD_STATS_REPLICAS of include/seld_hip.h; the test compares it with the library's

NAMES = [
    # hc_conv_kernel
    "edge_short_images_12x1",            # run-time taps, dstS = 17 < BP: the divide branch of decode; scalar stores
    "edge_straddle_6x1",                 # dstS >= BP: the wrap branch of decode
    "edge_wgrad_one_split_w28",          # run-time taps with 16-byte stores
    "r_3x3_c3_o3_n1_5x7_s22_cfg2x4",     # 3 channels; the strided data gradient
    "edge_ck24_4x4",                     # FAST 1x3, the channel tile straddles Cout / 2: mixed_wg in both modes
    "edge_dq_half_on_tile_6x1",          # FAST 1x1, Cout / 2 on a tile boundary: kbeg / kend alone
    "q_3x3_c16_o16_n1_5x7_cfg12x2",      # FAST 3x3, two position tiles per wave
    "r_1x1_c16_o128_n1_1x28",            # FAST 1x1 with 16-byte stores
    # hc_conv_vec_kernel
    "edge_vec_1x1_12x1",                 # 1x1 at KC 24, mixed_wg; forward pair with statistics on both slots
    "edge_vec_1x3_6x1",                  # 1x3 at KC 24; data-gradient pair
    "edge_vec_3x3_12x1",                 # 3x3 at KC 36
    "edge_vec_q_tail_6x1",               # padded channel rows, three position tiles and a tail
    "edge_wgrad_r_1x1_w64",              # data gradient: edge and interior workgroups; forward: 24 channels on hc_conv_kernel
    "edge_wgrad_tile_4_1_5_w28",         # 3x3 data gradient: edge and interior workgroups
    # hc_conv_smallk_kernel
    "dq_3x3_c8_o192_n2_128x128",         # <12, 3, 3>: the compile-time SPLIT form
    "dq_1x3_c8_o64_n2_128x128",          # a generic form
    "dq_1x5_c8_o64_n2_128x128",          # run-time taps
]
CASES = [X.case(n) for n in NAMES]

REQUIRED = {
    "general run-time taps fwd", "general run-time taps dgrad", "general FAST fwd", "general FAST dgrad",
    "general mixed_wg fwd", "general mixed_wg dgrad", "general several images per tile", "general scalar stores",
    "general 16-byte stores", "general channel tail",
    "vec 1x1 KC 24", "vec 1x3 KC 24", "vec 3x3 KC 36", "vec edge and interior", "vec mixed_wg", "vec forward pair",
    "vec 1x3 data-gradient pair",
    "smallk SPLIT", "smallk generic", "smallk run-time taps",
    "statistics digested", "forward pair statistics digested",
}


def _label(case, which):
    m = re.fullmatch(r"(\w+)<([\d, ]+)>", case["labels"][which])
    return m.group(1), [int(v) for v in m.group(2).split(",")]


def _geometry(case, which):
    """(Cdst, Ktot, dst extent) of the launch as fill_fwd / fill_dgrad set them."""
    kk = X.taps(case)
    if which == 0:
        return case["cout"], case["x"][1] * kk, X.out_extent(case)
    return case["x"][1], case["cout"] * kk, tuple(case["x"][2:])


def position_tiles(case, which):
    kernel, a = _label(case, which)
    if kernel == "hc_conv_smallk_kernel":
        return None
    _, _, (h, w) = _geometry(case, which)
    bp = a[1] * 64
    return (case["x"][0] * h * w + bp - 1) // bp


def digests_stats(case):
    """One workgroup per replica row and channel: the float atomics land on zeros, in no order that matters."""
    tiles = position_tiles(case, 0)
    return bool(case["stats"]) and tiles is not None and tiles <= STATS_REPLICAS


def traits(case):
    out = set()
    for which in (w for w in case["run"] if w < 2):
        kernel, a = _label(case, which)
        mode = "fwd" if which == 0 else "dgrad"
        cdst, ktot, (h, w) = _geometry(case, which)
        dst_s, ptot = h * w, case["x"][0] * h * w
        if kernel == "hc_conv_smallk_kernel":
            ct, kh, kw = a
            split = (ct, kh, kw) == (12, 3, 3) and ktot == 72 and dst_s % 64 == 0 and w % 64 == 0
            out.add("smallk SPLIT" if split else "smallk generic" if kh else "smallk run-time taps")
            continue
        ct, pt, kh, kw = a[:4]
        bc, bp = ct * 16, pt * 64
        unit = 16 if kernel == "hc_conv_kernel" else a[5]
        mixed = case["algebra"] == 8 and (ktot // 2) % unit == 0 and (cdst // 2) % 16 == 0 and ct % 2 == 0 and \
            (cdst // 2) % bc == bc // 2
        if kernel == "hc_conv_kernel":
            out.add(f"general {'FAST' if a[5] else 'run-time taps'} {mode}")
            if mixed:
                out.add(f"general mixed_wg {mode}")
            if dst_s < bp and ptot > dst_s:
                out.add("general several images per tile")
            out.add("general scalar stores" if dst_s % 4 else "general 16-byte stores")
            if cdst % 16:
                out.add("general channel tail")
            continue
        assert kernel == "hc_conv_vec_kernel", kernel
        out.add(f"vec {kh}x{kw} KC {a[5]}")
        if mixed:
            out.add("vec mixed_wg")
        pad_h, dil_h = X._two(case["padding"])[0], X._two(case["dilation"])[0]
        span = (max(pad_h, (kh - 1) * dil_h) + 1) * w
        edge = [p0 < span or p0 + bp + span > ptot for p0 in range(0, ptot, bp)]
        if any(edge) and not all(edge):
            out.add("vec edge and interior")
        if which == 0 and 0 in case["pair"] and (kh, kw) == (1, 1):
            out.add("vec forward pair")
            if digests_stats(case):
                out.add("forward pair statistics digested")
        if which == 1 and 1 in case["pair"] and (kh, kw) == (1, 3):
            out.add("vec 1x3 data-gradient pair")
    if 0 in case["run"] and digests_stats(case):
        out.add("statistics digested")
    return out


_covered = set().union(*(traits(c) for c in CASES))
assert REQUIRED <= _covered, sorted(REQUIRED - _covered)
assert all(c["kind"] == "conv" and c["stats"] for c in CASES)
assert all(not digests_stats(c) for c in CASES if _label(c, 0)[0] == "hc_conv_smallk_kernel")


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_case(P, case, dev):
    """{launch: tensor} of every launch of the case through the C entry points, under the environment already in force.
    Forward: bias; bias + addend; accumulate; bias + statistics (a small-K case: the first and the last, the other two
    epilogues are not that kernel's).  Data gradient: with the transposed-weight workspace, without one, from a workspace
    filled ahead.  Pairs: the forward pair with a different epilogue and statistics per slot, the data-gradient pair from
    weights and from workspaces filled ahead.  `... stats` entries are present where digests_stats() holds."""
    H, L = P.hip_ops, P._lib
    lib, st, d = L.lib(), L.current_stream(), X.desc(P.hip_ops, case)
    ref = ctypes.byref(d)
    host = X.inputs(case, "randn")
    t = {k: ([w.to(dev) for w in v] if isinstance(v, list) else v.to(dev)) for k, v in host.items()}
    keep_stats = digests_stats(case)
    out = {}

    def new_y():
        return torch.full(X.y_shape(case), float("nan"), device=dev)

    def new_stats():
        return torch.zeros(H.STATS_REPLICAS * 2 * case["cout"], device=dev)

    def workspace(n=1):
        nbytes = int(lib.seld_hc_conv_bwd_data_workspace(ref))
        return torch.empty(n * ((nbytes + 3) // 4), device=dev), n * nbytes

    def fwd(name, w, bias, y, epilogue, addend=None, stats=None):
        L.check(lib.seld_hc_conv_fwd_ex(ref, L.ptr(t["x"]), L.ptr_array8(t[w]), L.ptr(bias), L.ptr(y), epilogue, L.ptr(addend),
                                        L.ptr(stats), st), "seld_hc_conv_fwd_ex")
        out[name] = y
        if stats is not None and keep_stats:
            out[name + " stats"] = stats

    if 0 in case["run"]:
        smallk = _label(case, 0)[0] == "hc_conv_smallk_kernel"
        fwd("forward bias", "wA", t["biasA"], new_y(), 0)
        if not smallk:
            fwd("forward bias + addend", "wA", t["biasA"], new_y(), L.SELD_EPI_ADD, t["addA"])
            fwd("forward accumulate", "wA", None, t["target"].clone(), L.SELD_EPI_ACCUMULATE)
            fwd("forward bias + addend + statistics", "wA", t["biasA"], new_y(), L.SELD_EPI_ADD | L.SELD_EPI_STATS, t["addA"],
                new_stats())
        fwd("forward bias + statistics", "wA", t["biasA"], new_y(), L.SELD_EPI_STATS, None, new_stats())
    if 1 in case["run"]:
        dx = lambda: torch.full(tuple(case["x"]), float("nan"), device=dev)
        wsb, nbytes = workspace()
        out["data gradient with the workspace"] = dx()
        L.check(lib.seld_hc_conv_bwd_data_ex(ref, L.ptr(t["dy"]), L.ptr_array8(t["wA"]), L.ptr(out["data gradient with the workspace"]),
                                             L.ptr(wsb), nbytes, st), "seld_hc_conv_bwd_data_ex")
        out["data gradient without a workspace"] = dx()
        L.check(lib.seld_hc_conv_bwd_data(ref, L.ptr(t["dy"]), L.ptr_array8(t["wA"]), L.ptr(out["data gradient without a workspace"]),
                                          st), "seld_hc_conv_bwd_data")
        wts = []
        for w in ("wA", "wB"):
            wt, nbytes = workspace()
            L.check(lib.seld_hc_conv_transpose_weights(ref, L.ptr_array8(t[w]), L.ptr(wt), nbytes, st),
                    "seld_hc_conv_transpose_weights")
            wts.append(wt)
        out["data gradient from a workspace filled ahead"] = dx()
        L.check(lib.seld_hc_conv_bwd_data_wt(ref, L.ptr(t["dy"]), L.ptr(wts[0]),
                                             L.ptr(out["data gradient from a workspace filled ahead"]), st), "seld_hc_conv_bwd_data_wt")
        if 1 in case["pair"]:
            wsb, nbytes = workspace(2)
            out["data gradient of a pair"] = dx()
            L.check(lib.seld_hc_conv_pair_bwd_data(ref, L.ptr(t["dy"]), L.ptr(t["dyB"]), L.ptr_array8(t["wA"]), L.ptr_array8(t["wB"]),
                                                   L.ptr(out["data gradient of a pair"]), L.ptr(wsb), nbytes, st),
                    "seld_hc_conv_pair_bwd_data")
            out["data gradient of a pair from workspaces filled ahead"] = dx()
            L.check(lib.seld_hc_conv_pair_bwd_data_wt(ref, L.ptr(t["dy"]), L.ptr(t["dyB"]), L.ptr(wts[0]), L.ptr(wts[1]),
                                                      L.ptr(out["data gradient of a pair from workspaces filled ahead"]), st),
                    "seld_hc_conv_pair_bwd_data_wt")
    if 0 in case["pair"]:
        ya, yb, sa, sb = new_y(), t["target"].clone(), new_stats(), new_stats()
        L.check(lib.seld_hc_conv_pair_fwd(ref, L.ptr(t["x"]), L.ptr_array8(t["wA"]), L.ptr_array8(t["wB"]), L.ptr(t["biasA"]), None,
                                          L.ptr(ya), L.ptr(yb), L.SELD_EPI_ADD | L.SELD_EPI_STATS,
                                          L.SELD_EPI_ACCUMULATE | L.SELD_EPI_STATS, L.ptr(t["addA"]), None, L.ptr(sa), L.ptr(sb), st),
                "seld_hc_conv_pair_fwd")
        out["forward pair, slot 0: bias + addend + statistics"], out["forward pair, slot 1: accumulate + statistics"] = ya, yb
        if keep_stats:
            out["forward pair, slot 0 stats"], out["forward pair, slot 1 stats"] = sa, sb
    torch.cuda.synchronize()
    return out
