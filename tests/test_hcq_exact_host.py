"""Host side of the exact forward / data-gradient tests of the fast-product convolution (no GPU): the case table of
tests/golden/hcq_exact_cases.py reaches every launch of modes 0 and 1 that the dispatch fixture records, the built library
answers every case as listed, the edge shapes are the shapes they claim to be, and for every case the exactness argument
of tests/hcq_exact.py holds: the bound on the accumulators, an integer-valued float64 oracle, the statistics condition
as recorded.  Last, the comparison the GPU tests make notices the smallest things a kernel can get wrong."""
import json
import os

import pytest
import torch

from tests import hcq_exact as X
from tests.golden import hcq_exact_cases as C
from tests.golden import make_golden_hcq_dispatch as G
from tests.helpers import pkg

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hcq_dispatch.json")
IDS = [c["name"] for c in C.ALL_CASES]


def fixture_keys():
    """(mode, npair, label, slot kind) of every mode-0 / mode-1 launch in the fixture's `default` column."""
    with open(FIXTURE) as f:
        col = G.decode(json.load(f))["default"]
    keys = set()
    for a in col:
        if len(a) == 1:
            continue
        for (mode, npair), v in zip(G.COMBOS, a[1:1 + len(G.COMBOS)]):
            if mode in (0, 1) and v[1][0] == 0 and v[2][0] == 0:
                keys.add((mode, npair, v[1][1], v[2][5]))
    return keys


def table_keys(cases):
    return {(m, n, lab, slot) for c in cases for (m, n), (lab, slot) in c["launch"].items()}


def test_table_reaches_every_recorded_launch():
    want, have = fixture_keys(), table_keys(C.ALL_CASES)
    left_out = set(C.LEFT_OUT)
    print(f"{len(want)} launch keys of modes 0 and 1 in the fixture, {len(want & have)} reached by {len(C.ALL_CASES)} cases, "
          f"{len(left_out)} left out by name; {len(have - want)} further keys reached by the edge shapes")
    assert len(want) >= 100, "the fixture's default column was not read"
    assert left_out <= want and not (left_out & have), "a key is left out only while no case reaches it"
    assert all(isinstance(r, str) and len(r) > 20 for r in C.LEFT_OUT.values()), "every key left out has a written reason"
    assert 20 * len(left_out) <= len(want), "at most 5 % of the keys may be left out"
    assert want - have == left_out, sorted(want - have - left_out)
    # the key cases alone reach them: the edge shapes stand beside them
    assert want - table_keys(C.KEY_CASES) == left_out


@pytest.mark.parametrize("case", C.ALL_CASES, ids=IDS)
def test_library_answers_the_case_as_listed(case):
    P = pkg()
    d = X.desc(P.hip_ops, case)
    assert case["launch"], "a case without a launch checks nothing"
    for mode, npair in X.COMBOS:
        got = X.launch_key(P, d, mode, npair)
        assert got == case["launch"].get((mode, npair)), (case["name"], mode, npair, got)
        assert P.hip_ops._hcq_ok(d, mode, npair) == ((mode, npair) in case["launch"])
        if got is not None:
            assert P.hip_ops.hcq_label(d, mode, npair) == got[0]


def test_three_tile_cases_alone_are_large():
    """Only the three-tile keys need many positions (24 block channels of output and 512 position tiles, 256 for a
    forward pair); every other key case stays at a few hundred positions."""
    for c in C.KEY_CASES:
        progs = {X.tile_program(lab) for lab, _ in c["launch"].values()}
        if X.positions(c) > 1024:
            assert (1, 2, 2, False) in progs, c["name"]
            assert X.positions(c) in (16384, 32768) and 8 <= c["x"][1] <= 192, c["name"]
        if (1, 2, 2, False) in progs:
            assert X.positions(c) >= 16384


def _edges(kind):
    return [c for c in C.EDGE_CASES if c["edge"] == kind]


def test_edge_shapes_are_what_they_claim():
    P = pkg()
    H = P.hip_ops
    one = _edges("one_tile")
    assert one and all(X.positions(c) == 64 for c in one) and {len(c["k"]) for c in one} == {1, 2}
    assert any(c["x"][0] == 1 for c in _edges("n1")) and all(c["x"][0] == 3 for c in _edges("n3")) and len(_edges("n3")) >= 3
    for kind, h in (("h1", 1), ("h2", 2)):
        got = _edges(kind)
        assert {c["algebra"] for c in got} == {4, 8}
        assert all(c["k"] == (3, 3) and c["x"][2] == h for c in got)
    side = _edges("side_taps_in_padding")
    assert {c["algebra"] for c in side} == {4, 8}
    assert all(c["k"] == (3,) and c["dilation"] >= 64 and c["x"][2] == 64 for c in side)
    # the largest dilation each 1x3 row of the instantiation table takes and the first of the next row: every dilation in
    # between (there is a gap where no row takes the shape) is refused, and the row changes across it
    row = lambda c: c["launch"][C.FWD][0].split(", ")[2:7:4]         # (IBC, XI)
    for A in (4, 8):
        last = sorted((c for c in _edges("last_dilation_of_row") if c["algebra"] == A), key=lambda c: c["dilation"])
        first = sorted((c for c in _edges("first_dilation_of_row") if c["algebra"] == A), key=lambda c: c["dilation"])
        assert len(last) == len(first) + 1 >= 2
        for a, b in zip(last, first):
            assert a["dilation"] < b["dilation"] and row(a) != row(b), (a["name"], b["name"])
            for dil in range(a["dilation"] + 1, b["dilation"]):
                assert not H._hcq_ok(X.desc(H, dict(a, dilation=dil, padding=dil)), 0), (a["name"], dil)
        top = last[-1]
        assert not H._hcq_ok(X.desc(H, dict(top, dilation=top["dilation"] + 1, padding=top["dilation"] + 1)), 0)
    assert all(n in C.BY_NAME for n in C.GUARD + C.ROUTES)
    progs = {X.tile_program(C.BY_NAME[n]["launch"][C.FWD][0]) for n in C.GUARD}
    assert progs == set(X.TILE_PROGRAMS), "a guard-band case per tile program, mixed and first-layer kernels included"
    assert any(C.BY_NAME[n]["dilation"] >= 64 for n in C.GUARD)


@pytest.mark.parametrize("case", C.ALL_CASES, ids=IDS)
def test_exactness_bound_integer_oracle_and_statistics_condition(case):
    X.assert_exactness_bound(case)
    t = X.inputs(case)
    for n, v in t.items():
        for u in (v if isinstance(v, list) else [v]):
            assert u.dtype == torch.float32 and bool((u == u.round()).all())
            assert float(u.abs().max()) <= (1.0 if n in ("wA", "wB", "wS") else 2.0), n
    assert all(tuple(w.shape) == X.weight_shape(case) for w in t["wA"] + t["wB"]) and len(t["wA"]) == case["algebra"]
    assert all(float(w.abs().max()) == 1.0 for w in t["wA"] + t["wB"]), "thinning left a component without a weight"
    r = X.exact_oracle(case)                               # (asserts integer values inside the bound)
    assert tuple(r["yA"].shape) == X.y_shape(case) and tuple(r["dx"].shape) == tuple(case["x"])
    assert all(v.dtype == torch.int16 for v in r.values())
    assert bool((r["yA"] != r["yB"]).any()) and bool((r["dx"] != r["dx_pair"]).any()), "the two sets of a pair differ"
    # the bound leaves the half visible next to the largest value of any case, the statistics limit the one
    big = torch.tensor([float(3 * 8 * X.terms(case) + 6)], dtype=torch.float32)
    assert float((big + 0.5) - big) == 0.5
    assert X.stats_condition(case) == case["stats_exact"], case["name"]
    assert (t["wS"] is t["wA"]) == (case["thin"] == 1)
    assert all(float(w.abs().max()) == 1.0 for w in t["wS"]), "thinning left a component without a weight"


def test_every_tile_program_has_a_case_with_exact_statistics():
    have = {}
    for c in C.ALL_CASES:
        if C.FWD in c["launch"] and c["stats_exact"]:
            have.setdefault(X.tile_program(c["launch"][C.FWD][0]), c["name"])
        if C.FWD_PAIR in c["launch"] and c["stats_exact"]:
            have.setdefault(("pair",) + tuple([X.tile_program(c["launch"][C.FWD_PAIR][0])]), c["name"])
    for prog, what in X.TILE_PROGRAMS.items():
        assert prog in have, what
        if prog != "first":
            assert ("pair", prog) in have, what
    lim = torch.tensor([float(X.STATS_LIMIT - 1)], dtype=torch.float32)
    assert float((lim + 1.0) - lim) == 1.0


# ---- sensitivity ---------------------------------------------------------------------------------------------------------
def test_the_comparison_notices_a_dropped_tap_and_a_neighbours_halo():
    """The oracle differs from a copy of itself in which one tap of one channel is dropped, and from one whose halo
    columns come from the neighbouring batch item instead of the padding; assert_exact notices either, and a half, a NaN
    and an unwritten element."""
    case = X.case("dq_1x3_ib8_ob24_d5_n3_w128")
    t, r = X.inputs(case), X.exact_oracle(case)
    X.assert_exact("unchanged", r["yA"].clone(), r["yA"])
    # one tap of one (output, input) block channel of one component
    idx = tuple(t["wA"][2].nonzero()[0].tolist())
    ws = [w.clone() for w in t["wA"]]
    ws[2][idx] = 0.0
    dropped = X.conv64(case, t["x"], ws)
    assert 0 < int((dropped != r["yA"].double()).sum()) < dropped.numel()
    with pytest.raises(AssertionError, match=r"elements differ"):
        X.assert_exact("dropped tap", dropped.float(), r["yA"])
    # halo taken from the neighbour: the batch items laid end to end in one row, convolved, cut apart again
    N, Cc, Wd = case["x"]
    row = t["x"].permute(1, 0, 2).reshape(1, Cc, N * Wd)
    joined = X.conv64(dict(case, x=(1, Cc, N * Wd)), row, t["wA"]).view(case["cout"], N, Wd).permute(1, 0, 2)
    diff = (joined != r["yA"].double()).nonzero()
    d = case["dilation"]
    assert len(diff) and all(w < d or w >= Wd - d for w in diff[:, 2].tolist()), "only the halo columns differ"
    assert bool((joined[:, :, d:Wd - d] == r["yA"].double()[:, :, d:Wd - d]).all())
    with pytest.raises(AssertionError, match=r"elements differ"):
        X.assert_exact("neighbour's halo", joined.float(), r["yA"])
    for what, delta in (("a half", 0.5), ("one product", -1.0), ("NaN", float("nan"))):
        bad = r["dx"].float()
        bad[1, 7, 5] += delta
        with pytest.raises(AssertionError, match=r"1 of \d+ elements differ\n  \(1, 7, 5\)"):
            X.assert_exact(what, bad, r["dx"])
    # an element a launch did not write keeps the sentinel, which is no result; a write outside the view is seen
    out, buf, band = X.sentinel_output(X.y_shape(case), X.guard_band(case), "cpu")
    out.copy_(r["yA"])
    X.assert_band_intact("untouched", buf, band)
    out[0, 0, 0] = -7777.25
    with pytest.raises(AssertionError, match="1 of"):
        X.assert_exact("unwritten", out, r["yA"])
    buf[band - 1] = 0.0
    with pytest.raises(AssertionError, match="1 floats next to the output"):
        X.assert_band_intact("written before the view", buf, band)
    # statistics: exact where the condition holds, and then one count off is noticed
    o = X.stats_output(case)
    assert X.sums_are_exact(o)
    s1, s2 = X.channel_sums(o)
    rep = torch.zeros(4, 2 * case["cout"])
    rep[1, :case["cout"]], rep[3, case["cout"]:] = s1.float(), s2.float()
    assert X.assert_stats("split over replicas", rep, o, 4) is True
    rep[2, 5] += 1.0
    with pytest.raises(AssertionError, match=r"sum \(exact\): 1 of"):
        X.assert_stats("one off", rep, o, 4)
    assert not X.sums_are_exact(o * 4096.0)
