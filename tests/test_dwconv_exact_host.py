"""Host side of the exact tests of the depthwise convolution (no GPU): dw_plan restated in tests/dwconv_exact.py agrees
with the built library on the whole search grid and on every case -- seld_dwconv_kernel_label on (nr, div, staged),
seld_dwconv_bwd_weight_workspace = Cdst * (KK + 1) * N * tiles * 4 on the tile --, the case table names every plan the
grid meets and all 16 labels, the exactness argument holds for every case, and the table holds the edges it claims."""
import ctypes

import pytest
import torch

from tests import dwconv_exact as X
from tests.golden import dwconv_exact_cases as C
from tests.helpers import pkg

IDS = [c["name"] for c in C.ALL_CASES]
ALL_LABELS = {X.label_of(w, nr, div, st) for w in (0, 1, 2) for nr in (1, 4) for div in ((False, True) if w == 1 else (False,))
              for st in (False, True)}


def library_labels(P, case):
    H = P.hip_ops
    d = X.desc(H, case)
    return {w: H.dwconv_label(d, w) for w in (0, 1, 2)}


def _table_plans(cases):
    return {(w,) + tuple(p) for c in cases for w, p in c["plans"].items()}


def test_plan_restated_on_the_grid_and_table_names_every_plan():
    P = pkg()
    H, lib = P.hip_ops, P._lib.lib()
    met, labels, n = set(), set(), 0
    for c in X.grid():
        d = X.desc(H, c)
        assert c["x"][2] * c["x"][3] < 50000
        assert int(lib.seld_dwconv_bwd_weight_workspace(ctypes.byref(d))) == X.workspace_bytes(c), c
        for w in (0, 1, 2):
            got = H.dwconv_label(d, w)
            assert got == X.label(c, w), (c, w, got, X.label(c, w))
            labels.add(got)
            met.add((w,) + X.plan_key(c, w))
        n += 1
    print(f"{n} descriptors: {len(met)} plans (entry point, nr, div, staged, WC, candidate), {len(labels)} labels")
    assert len(ALL_LABELS) == 16 and labels == ALL_LABELS
    assert len(met) == 62
    assert met <= _table_plans(C.KEY_CASES), sorted(met - _table_plans(C.KEY_CASES))
    assert {lab for c in C.KEY_CASES for lab in c["labels"].values()} == ALL_LABELS
    # plan forms beyond the label
    assert {p[4] for p in met} == {1, 2, 4} and {p[5] for p in met} == {0, 1, 2}
    assert (1, 1, True, False, 2, 0) in met, "unstaged + phase map + WC = 2"
    assert any(p[3] and p[5] == 2 for p in met), "staged through the third candidate"


def test_every_staged_plan_has_a_case_that_can_run_both_staging_forms():
    """vec = 1 needs a source width divisible by 4 (and an aligned pointer, which the GPU test gives and takes away)."""
    for plan in sorted(p for p in _table_plans(C.KEY_CASES) if p[3]):
        assert any(tuple(c["plans"][plan[0]]) == plan[1:] and X.vec_possible(c, plan[0]) for c in C.KEY_CASES), plan
    odd = [c for c in C.ALL_CASES for w in (0, 1, 2) if X.plan(c, w)["staged"] and X.plan(c, w)["src_w"] % 4]
    assert odd, "staged launches on a width that is no multiple of 4"


@pytest.mark.parametrize("case", C.ALL_CASES, ids=IDS)
def test_library_answers_the_case_as_listed(case):
    P = pkg()
    H, lib = P.hip_ops, P._lib.lib()
    assert len(case["why"]) > 4 and set(case["plans"]) == set(case["labels"]) == {0, 1, 2}
    assert library_labels(P, case) == case["labels"]
    d = X.desc(H, case)
    for w in (0, 1, 2):
        assert X.plan_key(case, w) == tuple(case["plans"][w]), (w, X.plan_key(case, w))
        nr, div, staged, _, _ = case["plans"][w]
        assert X.label_of(w, nr, div, staged) == case["labels"][w]
    assert int(lib.seld_dwconv_bwd_weight_workspace(ctypes.byref(d))) == X.workspace_bytes(case)
    o = H.dwconv_out_shape(d)
    assert tuple(o) == X.out_extent(case)


@pytest.mark.parametrize("case", C.ALL_CASES, ids=IDS)
def test_exactness_bound_and_integer_oracle(case):
    X.assert_exactness_bound(case)
    fwd, wgrad = X.bounds(case)
    o = X.out_extent(case)
    assert fwd == case["m"] * X.taps(case) * 2 + 3 and wgrad == 4 * case["x"][0] * o[0] * o[1] + 1 < 2 ** 22
    big = torch.tensor([float(wgrad)], dtype=torch.float32)
    assert float((big + 0.25) - big) == 0.25
    t = X.inputs(case)
    for n, v in t.items():
        assert v.dtype == torch.float32 and bool((v == v.round()).all())
        assert float(v.abs().max()) <= {"w": 1.0, "bias": 3.0}.get(n, 2.0), n
    assert tuple(t["w"].shape) == X.weight_shape(case) and tuple(t["dy"].shape) == X.y_shape(case)
    r = X.exact_oracle(case)
    m = X.read_mask(case)
    assert bool((r["dx"][..., ~m] == 0.0).all()) if X.ndim(case) == 2 else bool((r["dx"][..., ~m[0]] == 0.0).all())


def test_the_table_holds_the_edges_it_claims():
    by = C.BY_NAME
    assert {c["m"] for c in C.ALL_CASES} >= {1, 2, 3} and by["e_c1"]["x"][1] == 1
    q = X.plan(by["e_tile_tail_both"], 0)
    assert q["dst"][0] % q["TH"] and q["dst"][1] % q["TW"] and q["dst"][0] > q["TH"]
    q = X.plan(by["e_tiles_w2"], 0)
    assert q["TW"] < q["dst"][1] < 2 * q["TW"]
    assert X.out_extent(by["e_out_1x1"]) == (1, 1)
    c = by["e_pad_km1"]
    assert tuple(c["padding"]) == tuple(k - 1 for k in c["k"])
    assert sum(1 for c in C.ALL_CASES if X.ndim(c) == 1) >= 4
    strides = {X.geometry(c)[2] for c in C.ALL_CASES}
    assert {(2, 1), (1, 2), (3, 3), (2, 2)} <= strides
    # the phase map of the data gradient: dilation divisible by the stride and not
    dms = {dm for c in C.ALL_CASES if X.plan(c, 1)["div"] for dm, s in zip(X.plan(c, 1)["dm"], X.geometry(c)[2]) if s > 1}
    assert {0, 1, 2} <= dms
    assert X.plan(by["e_m3_s2"], 1)["div"] and by["e_m3_s2"]["m"] == 3, "the phase map restages per output channel"
    assert not X.plan(by["e_m2_unstaged"], 1)["staged"] and by["e_m2_unstaged"]["m"] == 2


@pytest.mark.parametrize("name", ["e_m3_s2", "e_1d_k5_s2_m2"])
def test_the_comparison_notices_a_dropped_tap(name):
    case = X.case(name)
    t, r = X.inputs(case), X.exact_oracle(case)
    idx = tuple(t["w"].nonzero()[0].tolist())
    dropped = dict(t, w=t["w"].clone())
    dropped["w"][idx] = 0.0
    rd = X.oracle(case, dropped)
    for n in ("y", "dx"):
        assert 0 < int((rd[n] != r[n]).sum()) < r[n].numel()
        with pytest.raises(AssertionError, match=r"elements differ"):
            X.assert_exact("dropped tap, " + n, rd[n].float(), r[n])
    bad = (r["dw"] + 0.25).float()
    X.assert_exact("unchanged", bad, r["dw"] + 0.25)
    bad.view(-1)[1] += 0.25
    with pytest.raises(AssertionError, match=r"1 of \d+ elements differ"):
        X.assert_exact("a quarter", bad, r["dw"] + 0.25)
