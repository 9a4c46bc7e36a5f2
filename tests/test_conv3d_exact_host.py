"""Host side of the exact tests of the 3-D convolution family (no GPU): the case table of
tests/golden/conv3d_exact_cases.py reaches every label a descriptor can reach -- the two <2,4> labels of LEFT_OUT are
answered by no descriptor of a search over Co = 4..512 and up to 4 * 10^5 positions --, the built library answers every
case as listed, the restated tile choice and weight-gradient plan of tests/conv3d_exact.py agree with the library (labels;
workspace bytes = (nsplit * Co * Kc + nbias * C) * 4), the exactness argument holds for every case from its own numbers,
the table holds the edges it claims, and descriptors past the phase tables, the tap limit and 32-bit addressing are
refused by every entry point before anything is touched."""
import ctypes
import itertools

import pytest
import torch

from tests import conv3d_exact as X
from tests.golden import conv3d_exact_cases as C
from tests.helpers import pkg

EINVAL, EUNSUPPORTED = -1, -4            # include/seld_hip.h
IDS = [c["name"] for c in C.ALL_CASES]
GEMM_LABELS = {f"hc_conv3d_{k}_kernel<{ct}, {pt}>" for k in ("fwd", "phase") for ct, pt in X.TILES}
ALL_LABELS = GEMM_LABELS | {"hc_conv3d_wgrad_kernel"}


def library_labels(P, case):
    H = P.hip_ops
    d, op = X.desc(H, case)
    return {w: H.conv3d_label(d, op, w) for w in case["run"]}


def _probe(kind, Co, positions):
    """One tap, 4 reduction channels, `positions` output positions of one image: only Co and the position count decide."""
    return dict(name="probe", kind=kind, algebra=4, x=(1, 4, 1, 1, positions), cout=Co, k=(1, 1, 1), stride=(1, 1, 1),
                padding=(0, 0, 0), dilation=(1, 1, 1), output_padding=(0, 0, 0), run=(0,))


def test_tile_choice_restated_and_the_2x4_labels_unreachable():
    """c3_cfg restated in tests/conv3d_exact.py against the built library on the search grid of the cap: Co = 4..512 in
    steps of 4, position counts up to 4.2 * 10^5 (dense around the thresholds of every tile), both GEMM kernels."""
    H = pkg().hip_ops
    grid = sorted(set(itertools.chain(range(1, 72, 7), range(64, 4096, 331), range(4096, 110000, 2111),
                                      range(110000, 430000, 15503))))
    assert grid[-1] >= 400000
    seen = set()
    for kind in ("conv", "tconv"):
        for Co in range(4, 516, 4):
            for pos in grid:
                c = _probe(kind, Co, pos)
                d, op = X.desc(H, c)
                got = H.conv3d_label(d, op, 0)
                assert got == X.label(c, 0), (kind, Co, pos, got, X.label(c, 0))
                seen.add(got)
    print(f"{2 * 128 * len(grid)} descriptors, labels met: {sorted(seen)}")
    assert GEMM_LABELS - seen == set(C.LEFT_OUT), "LEFT_OUT is exactly what the search does not meet"
    # why: for Co <= 32 the candidate ties {4,4} and the earlier candidate keeps the tie
    for Co in (4, 16, 32):
        assert Co / 32.0 * 0.45 == Co / 64.0 * 0.9


def test_table_reaches_every_reachable_label():
    have = {lab for c in C.ALL_CASES for lab in c["labels"].values()}
    keys = {lab for c in C.KEY_CASES for lab in c["labels"].values()}
    assert sorted(C.LEFT_OUT) == sorted(f"hc_conv3d_{k}_kernel<2, 4>" for k in ("fwd", "phase"))
    assert have == ALL_LABELS - set(C.LEFT_OUT) and len(have) == 9
    assert keys == have, "the key cases alone reach them: the edge shapes stand beside them"
    # every (entry point, algebra, tile) of the key list
    got = {(c["kind"], w, c["algebra"], lab) for c in C.KEY_CASES for w, lab in c["labels"].items()}
    for kind, algs in (("conv", (1, 4, 8)), ("tconv", (1, 4))):
        for A in algs:
            assert (kind, 2, A, "hc_conv3d_wgrad_kernel") in got
            for w in (0, 1):
                stem = "hc_conv3d_phase_kernel" if (w == 1) != (kind == "tconv") else "hc_conv3d_fwd_kernel"
                for ct, pt in ((12, 1), (4, 4), (4, 1), (1, 4)):
                    assert (kind, w, A, f"{stem}<{ct}, {pt}>") in got, (kind, w, A, ct, pt)


@pytest.mark.parametrize("case", C.ALL_CASES, ids=IDS)
def test_library_answers_the_case_as_listed(case):
    P = pkg()
    H, lib = P.hip_ops, P._lib.lib()
    assert case["labels"] and case["run"] == tuple(sorted(case["labels"])) and len(case["why"]) > 4
    assert len(case["x"]) == 5 and case["x"][1] % case["algebra"] == 0 and case["cout"] % case["algebra"] == 0
    assert library_labels(P, case) == case["labels"]
    assert {w: X.label(case, w) for w in case["run"]} == case["labels"], "the restatement agrees"
    d, op = X.desc(H, case)
    assert H.conv3d_out_shape(d, op) == X.out_extent(case)
    if X.is_tconv(case):
        assert case["algebra"] in (1, 4)
        nbytes = lib.seld_hc_conv3d_transpose_bwd_weight_workspace(ctypes.byref(d), op)
    else:
        nbytes = lib.seld_hc_conv3d_bwd_weight_workspace(ctypes.byref(d))
    pl = X.wgrad_plan(case)
    assert int(nbytes) == pl["bytes"] == (pl["nsplit"] * pl["Co"] * pl["Kc"] + pl["nbias"] * case["cout"]) * 4


def test_weight_gradient_plan_restated_on_a_grid():
    """c3_plan / c3_bias_plan against the workspace queries: every regime of min(1024 / tiles, Ptot / 256, memory)."""
    H, lib = pkg().hip_ops, pkg()._lib.lib()
    n = 0
    regimes = set()
    for A, ci, co, k, N, sp in itertools.product((1, 4, 8), (8, 24, 136), (8, 72, 200), ((1, 1, 1), (2, 3, 2), (3, 3, 3)),
                                                 (1, 3), ((1, 2, 3), (2, 5, 7), (4, 9, 11), (5, 16, 17), (8, 33, 35), (9, 64, 80))):
        c = dict(name="grid", kind="conv", algebra=A, x=(N, ci) + sp, cout=co, k=k, stride=(1, 1, 1), padding=(1, 1, 1),
                 dilation=(1, 1, 1), run=(2,))
        d, _ = X.desc(H, c)
        pl = X.wgrad_plan(c)
        assert int(lib.seld_hc_conv3d_bwd_weight_workspace(ctypes.byref(d))) == pl["bytes"], (c, pl)
        regimes.add((pl["nsplit"] == 1, pl["nsplit"] == (pl["Ptot"] + 255) // 256, pl["nbias"] > 1))
        n += 1
        if A != 8:
            t = dict(c, kind="tconv", stride=(2, 1, 2), padding=(0, 0, 0), output_padding=(1, 0, 0))
            d, op = X.desc(H, t)
            pl = X.wgrad_plan(t)
            assert int(lib.seld_hc_conv3d_transpose_bwd_weight_workspace(ctypes.byref(d), op)) == pl["bytes"], (t, pl)
            n += 1
    print(f"{n} descriptors, regimes (one split, split by length, several bias blocks): {sorted(regimes)}")
    assert len(regimes) >= 5


@pytest.mark.parametrize("case", C.ALL_CASES, ids=IDS)
def test_exactness_bound_and_integer_oracle(case):
    X.assert_exactness_bound(case)
    fwd, dgrad, wgrad, dbias = X.bounds(case)
    A, cin, cout, KK = case["algebra"], case["x"][1], case["cout"], X.taps(case)
    # the bounds from the case's own numbers: reduction channels * taps products of magnitude 2 (+ bias 3);
    # 4 * blocks * positions for a weight gradient, blocks counted from the oracle's table
    assert fwd == 2 * cin * KK + 3 < 2 ** 24 and dgrad == 2 * cout * KK < 2 ** 24
    positions = case["x"][0] * X.vol(case["x"][2:] if X.is_tconv(case) else X.out_extent(case))
    assert X.wgrad_plan(case)["Ptot"] == positions
    assert wgrad >= 4 * {1: 1, 4: 4, 8: 8}[A] * positions
    if 2 in case["run"]:
        assert wgrad < 2 ** 22 and dbias < 2 ** 22
        big = torch.tensor([float(wgrad)], dtype=torch.float32)
        assert float((big + 0.25) - big) == 0.25, "the quarter stays visible next to the largest weight gradient"
    big = torch.tensor([float(max(fwd, dgrad))], dtype=torch.float32)
    assert float((big + 1.0) - big) == 1.0
    t = X.inputs(case)
    for n, v in t.items():
        for u in (v if isinstance(v, list) else [v]):
            assert u.dtype == torch.float32 and bool((u == u.round()).all())
            assert float(u.abs().max()) <= {"ws": 1.0, "bias": 3.0}.get(n, 2.0), n
    assert all(tuple(w.shape) == X.weight_shape(case) for w in t["ws"]) and len(t["ws"]) == A
    assert all(float((w != 0).float().mean()) > 0.5 for w in t["ws"] if w.numel() >= 256), "dense weights"
    r = X.exact_oracle(case)                               # (asserts integer values inside the bounds)
    assert ("y" in r) == (0 in case["run"]) and ("dx" in r) == (1 in case["run"]) and ("dw" in r) == (2 in case["run"])
    if "dx" in r and not X.is_tconv(case):
        m = X.read_mask(case)
        assert bool((r["dx"][:, :, ~m] == 0.0).all()), "no output reads these samples"


def test_blocks_per_component_counted_from_the_oracle():
    from oracle.seld_oracle import block_table
    for A, want in ((1, 1), (4, 4), (8, 8)):
        count = [0] * A
        for row in block_table(A):
            for e in row:
                if e is not None:
                    count[e[0]] += 1
        assert max(count) == want == X.blocks_per_component(A)


def _cls(name, which):
    return X.classes(C.BY_NAME[name], which)


def test_the_table_holds_the_edges_it_claims():
    by = C.BY_NAME
    pos = lambda n, w: X.gemm_positions(by[n], w)
    # position tails per tile, images per tile
    for n, w, tile in (("w12_tail_vec", 0, "<12, 1>"), ("w12_n3_scalar", 0, "<12, 1>"), ("w44_co36_tail", 0, "<4, 4>"),
                       ("w44_cr36_n3", 0, "<4, 4>"), ("n41_n5_three_images", 0, "<4, 1>"), ("n14_n3_one_tile", 0, "<1, 4>"),
                       ("p12_dgrad_cr20", 1, "<12, 1>"), ("p44_tconv_co36", 0, "<4, 4>")):
        assert by[n]["labels"][w].endswith(tile), n
        assert pos(n, w) % (64 * int(tile[-2])), f"{n}: the last tile is part-filled"
    assert by["w12_tail_vec"]["x"][0] == 1 and by["w12_n3_scalar"]["x"][0] == 3 and by["w44_cr36_n3"]["x"][0] == 3
    assert X.vol(by["w12_n3_scalar"]["x"][2:]) % 64 and X.vol(by["w44_cr36_n3"]["x"][2:]) % 256, "tiles straddle two images"
    assert 2 * X.vol(by["n41_n5_three_images"]["x"][2:]) < 64 and by["n41_n5_three_images"]["labels"][0].endswith("<4, 1>")
    assert 3 * X.vol(by["n14_n3_one_tile"]["x"][2:]) < 256 and by["n14_n3_one_tile"]["labels"][0].endswith("<1, 4>")
    # channel tails
    for n, co in (("w12_co200", 200), ("w12_co68", 68)):
        assert by[n]["cout"] == co and by[n]["labels"][0] == "hc_conv3d_fwd_kernel<12, 1>"
    assert by["w44_co36_tail"]["cout"] == 36 and by["w44_co36_tail"]["labels"][0] == "hc_conv3d_fwd_kernel<4, 4>"
    assert {by[n]["x"][1] for n in ("w12_cr20", "w44_cr36_n3", "w12_r_cr5_k", "key_conv_q_fwd_12x1")} == {20, 36, 5, 4}
    assert by["w12_tconv_dgrad_cr36"]["cout"] == 36 and by["w12_tconv_dgrad_cr36"]["labels"][1] == "hc_conv3d_fwd_kernel<12, 1>"
    # dual quaternion: the half-reduction skip on every tile
    c = by["dq12_fwd_cr40"]
    assert c["algebra"] == 8 and c["cout"] == 384 and c["labels"][0].endswith("fwd_kernel<12, 1>") and c["x"][1] == 40
    assert ((c["x"][1] // 2) + 15) // 16 == 2 and (c["x"][1] + 15) // 16 == 3, "cb_hi = 2 of 3 blocks"
    c = by["dq44_fwd_co128"]
    assert c["algebra"] == 8 and c["cout"] == 128 and c["labels"][0].endswith("fwd_kernel<4, 4>")
    c = by["dq12_dgrad_cr40"]
    assert c["algebra"] == 8 and c["x"][1] == 384 and c["cout"] == 40 and c["labels"][1].endswith("phase_kernel<12, 1>")
    assert (c["cout"] // 2) >> 4 == 1, "cb_lo = 1"
    c = by["dq44_dgrad_cr8"]
    assert c["algebra"] == 8 and c["x"][1] == 128 and c["cout"] == 8 and c["labels"][1].endswith("phase_kernel<4, 4>")
    c = by["n41_dq_dgrad_half"]
    assert c["x"][1] == 128 and c["labels"][1].endswith("phase_kernel<4, 1>") and by["n41_dq_cr8"]["x"][1] == 8
    assert by["key_conv_dq_fwd_12x1"]["cout"] == 384 and by["key_conv_dq_fwd_12x1"]["x"][1] == 8
    # epilogue store forms
    assert by["w12_tail_vec"]["x"][4] % 4 == 0 and by["dq44_fwd_co128"]["x"][4] % 4 == 0 and by["geo_pad_gt_image"]["x"][4] % 4 == 0
    assert by["w12_n3_scalar"]["x"][4] % 4 and by["w44_co36_tail"]["x"][4] % 4
    c = by["p12_tconv_s2"]
    assert c["stride"][2] == 2 and len(_cls("p12_tconv_s2", 0)) == 2 and c["labels"][0].endswith("phase_kernel<12, 1>")
    # phase tables
    strides = {s for c in C.ALL_CASES for s in c["stride"]}
    assert {1, 2, 3, 16} <= strides and X.C3_MAXS == 16
    assert {(s, d) for c in C.ALL_CASES for s, d in zip(c["stride"], c["dilation"])} >= \
        {(2, 1), (2, 2), (2, 3), (3, 1), (3, 2), (3, 3)}
    for n, w in (("ph_gcd_empty_class", 1), ("ph_s323_d312", 1), ("ph_s16", 1), ("ph_tconv_s3k2", 0), ("ph_tconv_gcd_op", 0),
                 ("ph_tconv_s16", 0)):
        assert any(ps > 0 and taps == 0 for ps, taps, _ in _cls(n, w)), f"{n}: a class with positions that no tap reaches"
    assert any(ps == 0 for ps, _, _ in _cls("ph_q0_depth1", 1)) and by["ph_q0_depth1"]["x"][2] == 1, "q[r] = 0: r >= out"
    c = by["ph_tconv_s3k2"]
    assert all(s > d * (k - 1) + 1 for s, d, k in zip(c["stride"], c["dilation"], c["k"])), "stride past the kernel extent"
    for n, w in (("ph_s232_d123", 1), ("p12_dgrad_s2_k3", 1)):
        assert len({ps for ps, _, _ in _cls(n, w)}) > 1 and len({t for _, t, _ in _cls(n, w)}) > 1, "unequal classes"
    assert len(_cls("ph_s16", 1)) == 16 and len(_cls("ph_tconv_s16", 0)) == 16
    # forward geometry
    c = by["geo_pad_gt_image"]
    assert c["padding"][0] > c["x"][2]
    assert {(3, 1, 3), (1, 3, 3), (2, 3, 2)} <= {c["k"] for c in C.ALL_CASES}
    assert {(1, 2, 1), (2, 1, 3)} <= {c["dilation"] for c in C.ALL_CASES}
    # transposed output padding
    tc = [c for c in C.ALL_CASES if X.is_tconv(c)]
    assert any(c["output_padding"] == (0, 0, 0) and max(c["stride"]) > 1 for c in tc)
    assert any(sum(1 for e in c["output_padding"] if e) == 1 for c in tc)
    assert any(s <= op < d for c in tc for s, op, d in zip(c["stride"], c["output_padding"], c["dilation"]))
    # weight-gradient plan: these rest on the library through test_library_answers_the_case_as_listed
    pl = lambda n: X.wgrad_plan(by[n])
    assert pl("wg_one_split")["nsplit"] == 1 and pl("wg_one_split")["Ptot"] % 16 and pl("wg_one_split")["Wo"] < 16
    assert pl("wg_splits")["nsplit"] == 4 and pl("wg_tconv_splits")["nsplit"] == 3
    assert pl("wg_last_split_short")["nsplit"] == 17 and pl("wg_last_split_short")["last_split"] == 4
    assert pl("wg_wo3")["Wo"] == 3
    assert pl("wg_kc65")["Kc"] % 64 == 1 and pl("wg_kc63_co70")["Kc"] % 64 == 63 and pl("wg_kc63_co70")["Co"] % 64 == 6
    q = pl("wg_dq_skip")
    half_cols = (q["Ci"] // 2) * q["KK"]
    assert by["wg_dq_skip"]["algebra"] == 8 and q["Co"] >= 128 and q["ntn"] == 3
    assert 64 < half_cols < 128 and 128 >= half_cols, "column tile 1 straddles the zero quadrant, tile 2 lies inside"
    assert pl("wg_one_split")["nbias"] == 1 and pl("wg_nbias2")["nbias"] == 2 and pl("wg_nbias2")["Ptot"] > 4096


def test_refusals_by_every_entry_point_with_null_buffers():
    """One stride past C3_MAXS, more than 4096 taps, and a tile whose images lie past 32-bit byte offsets
    (c3_addressable): refused before any buffer is looked at."""
    L, H = pkg()._lib, pkg().hip_ops
    lib = L.lib()
    buf = ctypes.create_string_buffer(96)

    def calls(d, op):
        ref = ctypes.byref(d)
        return {"fwd": lib.seld_hc_conv3d_fwd(ref, None, None, None, None, None),
                "bwd_data": lib.seld_hc_conv3d_bwd_data(ref, None, None, None, None),
                "bwd_weight": lib.seld_hc_conv3d_bwd_weight_acc(ref, None, None, None, None, None, 0, None),
                "label": lib.seld_hc_conv3d_kernel_label(ref, 0, buf, 96),
                "t_fwd": lib.seld_hc_conv3d_transpose_fwd(ref, op, None, None, None, None, None),
                "t_bwd_data": lib.seld_hc_conv3d_transpose_bwd_data(ref, op, None, None, None, None),
                "t_bwd_weight": lib.seld_hc_conv3d_transpose_bwd_weight_acc(ref, op, None, None, None, None, None, 0, None),
                "t_label": lib.seld_hc_conv3d_transpose_kernel_label(ref, op, 1, buf, 96)}

    zero = (ctypes.c_int32 * 3)(0, 0, 0)
    for what, d in (("stride 17", H.make_conv3d_desc((1, 4, 4, 4, 40), 4, 4, 1, (1, 1, 17), 0, 1)),
                    ("4352 taps", H.make_conv3d_desc((1, 4, 20, 20, 20), 4, 4, (17, 16, 16), 1, 0, 1))):
        assert set(calls(d, zero).values()) == {EUNSUPPORTED}, (what, calls(d, zero))
        assert lib.seld_hc_conv3d_bwd_weight_workspace(ctypes.byref(d)) == 0
        assert lib.seld_hc_conv3d_transpose_bwd_weight_workspace(ctypes.byref(d), zero) == 0
    ok = H.make_conv3d_desc((1, 4, 4, 4, 40), 4, 4, 1, (1, 1, 16), 0, 1)
    assert lib.seld_hc_conv3d_kernel_label(ctypes.byref(ok), 0, buf, 96) == 0, "stride 16 itself is served"
    # c3_addressable: 3 images of 48 x 64 x 256 x 256 floats (each below 2^28 elements) under one 256-position tile --
    # the output has 4 positions per image -- span 2.4 * 10^9 bytes.  The forward GEMM of the convolution and the data
    # gradient of the transposed convolution that mirrors it stream that operand.
    big = H.make_conv3d_desc((3, 48, 64, 256, 256), 4, 4, (1, 16, 16), 16, 0, (1, 16, 16))
    assert H.conv3d_out_shape(big) == (4, 1, 1)
    got = calls(big, zero)
    assert got["fwd"] == EUNSUPPORTED and got["label"] == EUNSUPPORTED, got
    assert got["bwd_data"] == EINVAL and got["bwd_weight"] == EINVAL, "the other entry points stop at the null buffers"
    tw, op = H.conv3d_transpose_desc((3, 4, 4, 1, 1), 48, 4, (1, 16, 16), 16, 0, 15, (1, 16, 16))
    assert H.conv3d_out_shape(tw, op) == (64, 256, 256)
    got = calls(tw, op)
    assert got["t_bwd_data"] == EUNSUPPORTED and got["t_label"] == EUNSUPPORTED, got
    assert got["t_fwd"] == EINVAL and got["t_bwd_weight"] == EINVAL


# ---- sensitivity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ph_s232_d123", "ph_tconv_k4s2", "geo_taps_133"])
def test_the_comparison_notices_a_dropped_tap_and_a_shifted_sample(name):
    case = X.case(name)
    t, r = X.inputs(case), X.exact_oracle(case)
    X.assert_exact("unchanged", r["y"].clone().float(), r["y"])
    comp = case["algebra"] - 1
    idx = tuple(t["ws"][comp].nonzero()[0].tolist())
    dropped = dict(t, ws=[w.clone() for w in t["ws"]])
    dropped["ws"][comp][idx] = 0.0
    rd = X.oracle(case, dropped)
    for n in ("y", "dx"):
        assert 0 < int((rd[n] != r[n]).sum()) < r[n].numel()
        with pytest.raises(AssertionError, match=r"elements differ"):
            X.assert_exact("dropped tap, " + n, rd[n].float(), r[n])
    i = tuple(e // 2 for e in case["x"])
    j = i[:4] + (i[4] + 1,)
    shifted = dict(t, x=t["x"].clone())
    a, b = float(t["x"][i]), float(t["x"][j])
    if a == b:
        a = a + 1.0 if a < 2.0 else a - 1.0
    shifted["x"][i], shifted["x"][j] = b, a
    rs = X.oracle(case, shifted)
    with pytest.raises(AssertionError, match=r"elements differ"):
        X.assert_exact("shifted sample, y", rs["y"].float(), r["y"])
    with pytest.raises(AssertionError, match=r"elements differ"):
        X.assert_slots_exact("shifted sample, dw", [w.float() for w in rs["dw"]], r["dw"])
    X.assert_slots_exact("unchanged dw", [(w + X.FILL_STEP * (k + 1)).float() for k, w in enumerate(r["dw"])], r["dw"],
                         X.FILL_STEP)
    for what, delta in (("a quarter", 0.25), ("one product", -1.0), ("NaN", float("nan"))):
        bad = r["dx"].float()
        bad[0, 1, 0, 2, 1] += delta
        with pytest.raises(AssertionError, match=r"1 of \d+ elements differ\n  \(0, 1, 0, 2, 1\)"):
            X.assert_exact(what, bad, r["dx"])
    out, buf, band = X.sentinel_output(X.y_shape(case), X.guard_band(case), "cpu")
    out.copy_(r["y"])
    X.assert_band_intact("untouched", buf, band)
    out[0, 0, 0, 0, 0] = -7777.25
    with pytest.raises(AssertionError, match="1 of"):
        X.assert_exact("unwritten", out, r["y"])
    buf[band - 1] = 0.0
    with pytest.raises(AssertionError, match="1 floats next to the output"):
        X.assert_band_intact("written before the view", buf, band)
