"""Host side of the exact tests of the block-matrix convolution family (no GPU): the case table of
tests/golden/hc_exact_cases.py reaches every (query, label) pair that tests/golden/conv_dispatch.json records over all its
environments -- but for the pairs LEFT_OUT names with a reason --, the built library answers every case as listed under
the case's environment, and for every case the exactness argument of tests/hc_exact.py holds: the bounds, an
integer-valued float64 oracle inside them, the statistics condition.  Last, the comparison the GPU tests make notices
the smallest things a kernel can get wrong."""
import ctypes
import json
import os

import pytest
import torch

from tests import hc_exact as X
from tests.golden import hc_exact_cases as C
from tests.golden import make_golden_conv_dispatch as G
from tests.golden.conv_geometry_cases import untouched_mask
from tests.helpers import pkg

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_dispatch.json")
IDS = [c["name"] for c in C.ALL_CASES]
# answer column of the fixture -> (kind, which)
COLUMNS = {3: ("conv", 0), 4: ("conv", 1), 5: ("conv", 2), 10: ("tconv", 0), 11: ("tconv", 1), 12: ("tconv", 2)}
WHAT = {("conv", 0): "forward", ("conv", 1): "data gradient", ("conv", 2): "weight gradient",
        ("tconv", 0): "transposed forward", ("tconv", 1): "transposed data gradient",
        ("tconv", 2): "transposed weight gradient"}


def fixture_pairs():
    """(kind, which, label) of every answer in the six label columns, over all recorded environments."""
    with open(FIXTURE) as f:
        rec = G.decode(json.load(f))
    pairs = set()
    for col in rec.values():
        for a in col:
            if len(a) == 1:
                continue
            for f, q in COLUMNS.items():
                if a[f][0] == 0:
                    pairs.add(q + (a[f][1],))
    return pairs


def table_pairs(cases):
    return {(c["kind"], w, lab) for c in cases for w, lab in c["labels"].items()}


def set_case_env(case, seld_env):
    for k, v in case["env"].items():
        seld_env.set(k, v)
    pkg().hip_ops._drop_kernel_choice_caches()


def library_labels(P, case):
    """What the built library answers for the case's launches under the environment in force."""
    H, lib = P.hip_ops, P._lib.lib()
    buf = ctypes.create_string_buffer(96)
    got = {}
    for w in case["run"]:
        if X.is_tconv(case):
            d, op = X.desc(H, case)
            rc = lib.seld_hc_conv_transpose_kernel_label(ctypes.byref(d), op, w, buf, 96)
        else:
            rc = lib.seld_hc_conv_kernel_label(ctypes.byref(X.desc(H, case)), w, buf, 96)
        got[w] = buf.value.decode() if rc == 0 else f"rc {rc}"
    return got


def test_table_reaches_every_recorded_label():
    want, have = fixture_pairs(), table_pairs(C.ALL_CASES)
    left_out = set(C.LEFT_OUT)
    per_query = {q: len({p for p in want if p[:2] == q}) for q in COLUMNS.values()}
    print(f"{len(want)} (query, label) pairs in the fixture: " + ", ".join(f"{n} {WHAT[q]}" for q, n in per_query.items()))
    print(f"{len(want & have)} reached by {len(C.ALL_CASES)} cases, {len(left_out)} left out by name")
    for p in sorted(have - want):
        print(f"reached by a case and never recorded by the fixture: {WHAT[p[:2]]} {p[2]}")
    assert len(want) == 168 and per_query == {("conv", 0): 35, ("conv", 1): 28, ("conv", 2): 42, ("tconv", 0): 3,
                                              ("tconv", 1): 31, ("tconv", 2): 29}, "the fixture was not read as counted"
    assert left_out <= want and not (left_out & have), "a pair is left out only while no case reaches it"
    assert all(isinstance(r, str) and len(r) > 40 for r in C.LEFT_OUT.values()), "every pair left out has a written reason"
    assert 20 * len(left_out) <= 168, "at most 5 % of the pairs may be left out"
    assert want - have == left_out, sorted(want - have - left_out)
    assert want - table_pairs(C.KEY_CASES) == left_out, "the key cases alone reach them: the edge shapes stand beside them"
    # the question the fixture leaves open: the 8-channel-tile small-K instantiations are reachable
    extra = have - want
    assert {("conv", 0, f"hc_conv_smallk_kernel<8, {k}>") for k in ("0, 0", "1, 3", "3, 3")} <= extra


def test_pairs_left_out_need_the_dual_quaternion():
    """The reason LEFT_OUT gives, checked against the library: every descriptor that answers one of those labels for a
    transposed convolution's weight gradient is a dual quaternion one, and the transposed convolution refuses it."""
    P = pkg()
    H, lib = P.hip_ops, P._lib.lib()
    with open(FIXTURE) as f:
        rec = G.decode(json.load(f))
    rows = list(G.descriptors())
    seen = 0
    for (A, ci, co, k, s, d, p, hw, n), a in zip(rows, rec["default"]):
        if len(a) > 1 and ("tconv", 2, a[12][1]) in C.LEFT_OUT:
            assert A == 8, (A, ci, co, k)
            seen += 1
    assert seen > 0
    assert all(key[0] == "tconv" and key[1] == 2 and "<2, 3, 4, " in key[2] for key in C.LEFT_OUT)
    # the label query answers for such a descriptor; the entry point refuses it before anything reaches the device
    # (tests/test_gpu_tconv.py holds the library's own SELD_EUNSUPPORTED for it)
    d, op = H.conv_transpose_desc((1, 8, 4, 8), 8, 8, (3, 3), 1, 1, 0, 1)
    buf = ctypes.create_string_buffer(96)
    assert lib.seld_hc_conv_transpose_kernel_label(ctypes.byref(d), op, 2, buf, 96) == 0
    with pytest.raises(P._lib.SeldHipError):
        H.hyper_conv_transpose(torch.zeros(1, 8, 4, 8), [torch.zeros(1, 1, 3, 3)] * 8, None, 1, 1, 0, 1)


@pytest.mark.parametrize("case", C.ALL_CASES, ids=IDS)
def test_library_answers_the_case_as_listed(case, seld_env):
    P = pkg()
    H, lib = P.hip_ops, P._lib.lib()
    assert case["labels"] and case["run"] == tuple(sorted(case["labels"])) and len(case["why"]) > 4
    assert set(case["env"]) <= {"SELD_CONV_NO_HCQ", "SELD_CONV_CFG", "SELD_CONV_NO_SMALLK"}
    assert len(case["x"]) == 4 and set(case["pair"]) <= set(case["run"])
    assert 1 not in case["pair"] or 1 in case["run"]
    set_case_env(case, seld_env)
    assert library_labels(P, case) == case["labels"]
    out = (ctypes.c_int32 * 2)()
    if X.is_tconv(case):
        d, op = X.desc(H, case)
        assert case["algebra"] in (1, 4) and not case["pair"] and not case["stats"]
        assert lib.seld_hc_conv_transpose_out_shape(ctypes.byref(d), op, out) == 0
    else:
        d = X.desc(H, case)
        assert lib.seld_hc_conv_out_shape(ctypes.byref(d), out) == 0, "hc_validate accepts every case"
        assert tuple(int(lib.seld_hc_conv_pair_supported(ctypes.byref(d), w)) for w in (0, 1, 2)) == case["pair_ok"]
        assert all(case["pair_ok"][w] for w in case["pair"]), "a pair launch is listed only where the library runs one"
        if 0 in case["pair"]:
            assert case["labels"][0].startswith("hc_conv_vec_kernel<"), "forward pairs run on the vector-staging kernel alone"
        # under its environment the case stays in the block-matrix family from every entry point
        if case["algebra"] > 1:
            assert not any(H._hcq_ok(d, m, n) for m in (0, 1) for n in (1, 2)), case["name"]
            assert not H._hcq_wgrad_ok(d) and not H._hcq_wgrad_ok(d, 2) and H.wgrad_group_family(d) == -1, case["name"]
    assert (out[0], out[1]) == X.out_extent(case)


@pytest.mark.parametrize("case", C.ALL_CASES, ids=IDS)
def test_exactness_bound_and_integer_oracle(case):
    X.assert_exactness_bound(case)
    t = X.inputs(case)
    for n, v in t.items():
        for u in (v if isinstance(v, list) else [v]):
            assert u.dtype == torch.float32 and bool((u == u.round()).all())
            assert float(u.abs().max()) <= (1.0 if n in ("wA", "wB", "wS") else 2.0), n
    assert all(tuple(w.shape) == X.weight_shape(case) for w in t["wA"] + t["wB"]) and len(t["wA"]) == case["algebra"]
    r = X.exact_oracle(case)                               # (asserts integer values inside the bounds)
    assert tuple(r["yA"].shape) == X.y_shape(case)
    assert ("dx" in r) == (1 in case["run"]) and ("dwA" in r) == (2 in case["run"])
    assert ("dx_pair" in r) == (1 in case["pair"]) and ("dwB" in r) == (2 in case["pair"])
    if "dx" in r and not X.is_tconv(case):
        m = untouched_mask(case)
        assert bool((r["dx"][:, :, m] == 0.0).all()), "no output reads these samples"
    # the bounds leave the quarter visible next to the largest weight gradient, the one next to the largest output
    fwd, dgrad, wgrad, _ = X.bounds(case)
    big = torch.tensor([float(wgrad)], dtype=torch.float32)
    assert float((big + 0.25) - big) == 0.25
    big = torch.tensor([float(max(fwd, dgrad))], dtype=torch.float32)
    assert float((big + 1.0) - big) == 1.0
    if case["stats"]:
        assert 0 in case["run"] and X.statistics_condition(case), "a statistics case must meet the exactness condition"


def test_blocks_per_component_counted_from_the_sign_tables():
    from oracle.seld_oracle import block_table
    assert [X.blocks_per_component(A) for A in (1, 4, 8)] == [1, 4, 8]
    for A in (1, 4, 8):
        table = block_table(A)
        for p in range(A):
            for q in range(A):
                comp, zero, neg = X.hc_comp(A, p, q)
                assert (table[p][q] is None) == zero
                if not zero:
                    assert table[p][q] == (comp, -1 if neg else 1), (A, p, q)


def test_the_table_holds_the_edges_it_claims():
    by = C.BY_NAME
    stat = [c for c in C.ALL_CASES if c["stats"]]
    for stem in ("hc_conv_kernel<", "hc_conv_vec_kernel<", "hc_conv_smallk_kernel<"):
        assert any(c["labels"][0].startswith(stem) for c in stat), f"statistics on {stem}"
    for taps in ("0, 0", "1, 3", "3, 3"):
        assert any(c["labels"][0].endswith(f", {taps}>") and c["labels"][0].startswith("hc_conv_smallk") for c in stat)
    assert by["dq_3x3_c8_o64_n2_128x128_nosmallk"]["labels"][0].startswith("hc_conv_kernel<")
    for cfg in G.CONV_CFGS:
        ct, pt = (int(v) for v in cfg.split(","))
        T = f"_{ct}x{pt}"
        BP, BC = 64 * pt, 16 * ct
        pos = lambda n: X.y_shape(by[n])[0] * X.y_shape(by[n])[2] * X.y_shape(by[n])[3]
        img = lambda n: X.y_shape(by[n])[2] * X.y_shape(by[n])[3]
        for n in ("ptot_tail", "short_images", "straddle", "n1", "chan_tail", "k_tail", "ck6", "ck24", "pad_gt_image",
                  "stride2", "stride3", "dil_h", "dil_w", "taps_1x5", "taps_2x2", "dq_half_on_tile", "dq_half_off_tile"):
            c = by["edge_" + n + T]
            assert c["env"]["SELD_CONV_CFG"] == cfg
            for w in (0, 1):
                assert c["labels"][w].startswith(f"hc_conv_kernel<{ct}, {pt}, "), (c["name"], c["labels"][w])
        assert pos("edge_ptot_tail" + T) % BP and img("edge_short_images" + T) * 2 < BP
        assert img("edge_straddle" + T) >= BP and img("edge_straddle" + T) % BP
        assert by["edge_n1" + T]["x"][0] == 1 and by["edge_chan_tail" + T]["cout"] % BC and by["edge_chan_tail" + T]["x"][1] % BC
        assert by["edge_ck6" + T]["labels"][0].endswith("0, 0, 0, 0>") and by["edge_ck24" + T]["labels"][0].endswith("1, 3, 0, 1>")
        assert by["edge_ck6" + T]["labels"][1].endswith("0, 0, 1, 0>") and by["edge_ck24" + T]["labels"][1].endswith("1, 3, 1, 1>")
        assert (by["edge_dq_half_on_tile" + T]["cout"] // 2) % BC == 0 and (by["edge_dq_half_off_tile" + T]["cout"] // 2) % BC
        assert by["edge_pad_gt_image" + T]["padding"][1] > by["edge_pad_gt_image" + T]["x"][3]
    for cfg in ("12x1", "6x1"):
        assert by["edge_vec_1x1_" + cfg]["pair"] == (0, 1) and ", 24, " in by["edge_vec_1x1_" + cfg]["labels"][0]
        assert 1 in by["edge_vec_1x3_" + cfg]["pair"] and ", 36, " in by["edge_vec_3x3_" + cfg]["labels"][0]
    for W_, stem in ((28, "hc_wgrad_kernel<"), (36, "hc_wgrad32_kernel<"), (64, "hc_wgrad_row_kernel<")):
        for n in ("one_split", "splits", "s21", "p0", "dh2", "tile_4_1_5", "tile_4_1_10", "tile_4_3_5"):
            c = by[f"edge_wgrad_{n}_w{W_}"]
            assert c["labels"][2].startswith(stem), (c["name"], c["labels"][2])
            assert (2 in c["pair"]) == (W_ == 64), "the pair launch runs on the row kernel alone"
        assert X.positions(by[f"edge_wgrad_one_split_w{W_}"]) <= 512 < 2 * 512 < X.positions(by[f"edge_wgrad_splits_w{W_}"])
    tiles = {c["labels"][2].split("<")[1].rsplit(", ", 3 if "row" in c["labels"][2] else 2)[0]
             for c in C.ALL_CASES if 2 in c["labels"]}
    assert tiles == {"2, 4, 4", "4, 3, 5", "2, 2, 2", "2, 3, 4", "4, 1, 5", "4, 1, 10"}, tiles
    tc = [c for c in C.ALL_CASES if X.is_tconv(c)]
    assert {c["labels"][0] for c in tc if 0 in c["labels"]} == {f"hc_tconv_kernel<{t}>" for t in ("12, 1", "4, 4", "1, 4")}
    assert {(1, 1), (2, 2), (2, 1)} <= {c["stride"] for c in tc} and {(0, 0), (1, 1)} <= {c["output_padding"] for c in tc}
    o = by["edge_tconv_o_over"]
    mirror = dict(o, kind="conv", x=X.y_shape(o), cout=o["x"][1])
    assert X.out_extent(mirror)[0] > o["x"][2] and X.out_extent(mirror)[1] > o["x"][3], "o_over is smaller than the full output"


# ---- sensitivity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge_ck24_4x4", "edge_stride2_12x2", "edge_wgrad_splits_w36", "edge_tconv_s2_op1"])
def test_the_comparison_notices_a_dropped_tap_and_a_shifted_sample(name):
    """The oracle differs from a copy of itself in which one tap of one weight component is zeroed, and from one in which
    one input sample moved by one position; assert_exact notices either in every result the GPU tests compare."""
    case = X.case(name)
    t, r = X.inputs(case), X.exact_oracle(case)
    X.assert_exact("unchanged", r["yA"].clone().float(), r["yA"])
    # one tap of one (output, input) block channel of one component
    comp = case["algebra"] - 1
    idx = tuple(t["wA"][comp].nonzero()[0].tolist())
    dropped = dict(t, wA=[w.clone() for w in t["wA"]])
    dropped["wA"][comp][idx] = 0.0
    rd = X.oracle(case, dropped)
    for n in ("yA", "dx"):
        assert 0 < int((rd[n] != r[n]).sum()) < r[n].numel()
        with pytest.raises(AssertionError, match=r"elements differ"):
            X.assert_exact("dropped tap, " + n, rd[n].float(), r[n])
    # one sample of x moved by one position along W
    n_, c_, h_, w_ = (e // 2 for e in case["x"])
    assert t["x"].shape[3] > w_ + 1
    shifted = dict(t, x=t["x"].clone())
    a, b = float(t["x"][n_, c_, h_, w_]), float(t["x"][n_, c_, h_, w_ + 1])
    if a == b:
        a = a + 1.0 if a < 2.0 else a - 1.0
    shifted["x"][n_, c_, h_, w_], shifted["x"][n_, c_, h_, w_ + 1] = b, a
    rs = X.oracle(case, shifted)
    assert 0 < int((rs["yA"] != r["yA"]).sum()) < r["yA"].numel()
    with pytest.raises(AssertionError, match=r"elements differ"):
        X.assert_exact("shifted sample, y", rs["yA"].float(), r["yA"])
    changed = [i for i in range(case["algebra"]) if bool((rs["dwA"][i] != r["dwA"][i]).any())]
    assert changed
    with pytest.raises(AssertionError, match=r"elements differ"):
        X.assert_slots_exact("shifted sample, dw", [w.float() for w in rs["dwA"]], r["dwA"])
    X.assert_slots_exact("unchanged dw", [(w + X.FILL_STEP * (i + 1)).float() for i, w in enumerate(r["dwA"])], r["dwA"],
                         X.FILL_STEP)
    for what, delta in (("a quarter", 0.25), ("one product", -1.0), ("NaN", float("nan"))):
        bad = r["dx"].float()
        bad[0, 1, 0, 2] += delta
        with pytest.raises(AssertionError, match=r"1 of \d+ elements differ\n  \(0, 1, 0, 2\)"):
            X.assert_exact(what, bad, r["dx"])
    # an element a launch did not write keeps the sentinel, which is no result; a write outside the view is seen
    out, buf, band = X.sentinel_output(X.y_shape(case), X.guard_band(case), "cpu")
    out.copy_(r["yA"])
    X.assert_band_intact("untouched", buf, band)
    out[0, 0, 0, 0] = -7777.25
    with pytest.raises(AssertionError, match="1 of"):
        X.assert_exact("unwritten", out, r["yA"])
    buf[band - 1] = 0.0
    with pytest.raises(AssertionError, match="1 floats next to the output"):
        X.assert_band_intact("written before the view", buf, band)
    if case["stats"]:
        o = X.stats_output(case)
        s1, s2 = X.channel_sums(o)
        rep = torch.zeros(4, 2 * case["cout"])
        rep[1, :case["cout"]], rep[3, case["cout"]:] = s1.float(), s2.float()
        assert X.assert_stats("split over replicas", rep, o, 4) is True
        rep[2, 1] += 1.0
        with pytest.raises(AssertionError, match=r"sum \(exact\): 1 of"):
            X.assert_stats("one off", rep, o, 4)
