"""The extended event-list scoring without a GPU: what the two new entry points answer to arguments they refuse (nothing is
launched, so null pointers do), the header's constants against the Python ones, and the generator's conditions on the
committed fixture (tests/golden/event_metrics_ex.npz), recomputed by the numpy restatement."""
import ctypes
import inspect
import re

import numpy as np
import pytest

from tests import event_metrics_ex_helpers as XH
from tests.event_metrics_helpers import detection_counts, seld_scores
from tests.golden.event_metrics_ex_cases import EVENT_METRIC_EX_CASES, EX_CASE_IDS, assign_problems
from tests.helpers import pkg

EINVAL, EUNSUPPORTED = -1, -4
NULL = ctypes.c_void_p(0)


def _accumulate(lib, pred_count=0, true_count=0, recordings=1, n_frames=10, nb_classes=14, fpb=10, coords=3, max_tracks=3,
                out=NULL):
    return lib.seld_event_metrics_accumulate_ex(NULL, NULL, pred_count, NULL, NULL, true_count, recordings, n_frames, nb_classes,
                                                fpb, coords, max_tracks, 2.0, 20.0, out, out, out, NULL)


def test_accumulate_ex_refuses_without_launching():
    lib = pkg()._lib.lib()
    some = ctypes.c_void_p(64)                          # never dereferenced: every call below is refused before any launch
    for kw in (dict(coords=1), dict(coords=4), dict(coords=0), dict(max_tracks=0), dict(max_tracks=9), dict(max_tracks=-1),
               dict(nb_classes=65), dict(nb_classes=-1), dict(fpb=0), dict(recordings=-1), dict(pred_count=-1),
               dict(true_count=-1), dict(n_frames=-1), dict(pred_count=3), dict(true_count=3, coords=2, max_tracks=8)):
        assert _accumulate(lib, out=some, **kw) == EINVAL, kw
    assert _accumulate(lib) == EINVAL                   # no accumulators
    assert _accumulate(lib, out=some, pred_count=1 << 28, coords=2, max_tracks=8) == EUNSUPPORTED
    assert _accumulate(lib, out=some, true_count=1 << 28) == EUNSUPPORTED


def test_least_distance_refuses_without_launching():
    lib = pkg()._lib.lib()

    def call(problems, coords, p=NULL):
        return lib.seld_least_distance(p, p, p, p, problems, coords, p, p, p, p, NULL)
    some = ctypes.c_void_p(64)
    assert call(-1, 3, some) == EINVAL
    assert call(1, 4, some) == EINVAL and call(1, 1, some) == EINVAL
    assert call(1, 3) == EINVAL and call(5, 2) == EINVAL              # null pointers
    assert call(1 << 28, 3, some) == EUNSUPPORTED
    assert call(0, 3) == 0 and call(0, 2) == 0                        # no problem: nothing to read or write


def test_header_constants_and_prototypes():
    L, H, D = pkg()._lib, pkg().hip_ops, pkg().Dcase21_metrics
    with open(L.HEADER_PATH) as f:
        header = f.read()
    defines = dict(re.findall(r"^#define (SELD_EVENT_METRIC\w+) (\d+)$", header, flags=re.M))
    assert int(defines["SELD_EVENT_METRICS_MAX_TRACKS"]) == H.EVENT_METRICS_MAX_TRACKS == 3
    assert int(defines["SELD_EVENT_METRICS_MAX_TRACKS_EX"]) == H.EVENT_METRICS_MAX_TRACKS_EX == 8
    assert int(defines["SELD_EVENT_METRIC_COUNTERS"]) == len(H.EVENT_METRIC_COUNTERS)
    protos = L.prototypes(header)
    old, new = protos["seld_event_metrics_accumulate"][1], protos["seld_event_metrics_accumulate_ex"][1]
    assert len(old) == 16 and new == old[:10] + [ctypes.c_int32, ctypes.c_int32] + old[10:]
    assert len(protos["seld_least_distance"][1]) == 11
    assert list(inspect.signature(D.least_distance_between_gt_pred).parameters) == ["gt_list", "pred_list"]
    assert list(inspect.signature(D.SELDMetrics.__init__).parameters) == ["self", "doa_threshold", "nb_classes", "max_tracks"]
    sig = inspect.signature(H.score_events).parameters
    assert (sig["coords"].default, sig["max_tracks"].default, sig["flags"].default) == (3, 3, None)
    assert callable(H.assign_doas)
    for empty in (D.least_distance_between_gt_pred(np.zeros((0, 3)), np.zeros((4, 3))),
                  D.least_distance_between_gt_pred(np.zeros((2, 2)), np.zeros((0, 2)))):      # no device needed
        assert [a.shape for a in empty] == [(0,)] * 3 and empty[1].dtype.kind == "i"
    with pytest.raises(L.SeldHipError, match="8"):
        D.least_distance_between_gt_pred(np.zeros((9, 3)), np.zeros((1, 3)))


@pytest.mark.parametrize("case", EVENT_METRIC_EX_CASES, ids=EX_CASE_IDS)
def test_fixture_keeps_the_generators_conditions(case, golden):
    g, name = golden("event_metrics_ex"), case["name"] + "."
    info = {}
    dc, de = XH.score_case(case, info)
    XH.check_conditions(case, info)
    tol = float(g[name + "total_DE_tol"][0])
    assert dc == g[name + "dcase"].tolist()
    assert abs(de - float(g[name + "total_DE"][0])) <= tol
    assert tol == XH.total_de_tolerance(float(g[name + "total_DE"][0]), info["angles"])
    assert np.allclose(seld_scores(dc, de), g[name + "scores"], rtol=1e-12, atol=1e-12)
    sed = np.sum([detection_counts(p, t, case["n_frames"], case["spatial_threshold"])[1]
                  for p, t in zip(case["pred"], case["true"])], 0)
    assert sed.tolist() == g[name + "sed"].tolist()
    assert (name + "lsd" in g) == (case["coords"] == 3)
    if case["coords"] == 3:
        lsd = np.sum([detection_counts(p, t, case["n_frames"], case["spatial_threshold"])[0]
                      for p, t in zip(case["pred"], case["true"])], 0)
        assert lsd.tolist() == g[name + "lsd"].tolist()
    rows = max(int(np.sum(r[:, 0] // case["fpb"] == b)) for r in case["pred"] + case["true"] for b in np.unique(r[:, 0] // case["fpb"]))
    assert (rows > 256) == (case["name"] == "cart_dense")           # the one case that leaves the staged path
    assert info["cell"] == {"sph_general": 3, "sph_degenerate": 2, "ties": 6, "ties_cart": 6}.get(case["name"], 8)


@pytest.mark.parametrize("spherical", [False, True], ids=["cart", "sph"])
def test_assign_fixture_is_unique_and_well_separated(spherical, golden):
    g, tag = golden("event_metrics_ex"), "assign.sph." if spherical else "assign.cart."
    gt, pred, gn, qn = assign_problems(spherical)
    assert sorted(zip(gn.tolist(), qn.tolist())) == [(a, b) for a in range(9) for b in range(9)]
    for b in range(81):
        n = min(int(gn[b]), int(qn[b]))
        assert int(g[tag + "pairs"][b]) == n and (g[tag + "row"][b, n:] == -1).all() and (g[tag + "col"][b, n:] == -1).all()
        if n == 0:
            continue
        cost = XH.cost_matrix(gt[b, :gn[b]], pred[b, :qn[b]])
        rows, cols, lead, tie = XH.best_assignment(cost)
        assert tie is None and lead >= XH.LEAD
        assert rows == g[tag + "row"][b, :n].tolist() and cols == g[tag + "col"][b, :n].tolist()
        ref = g[tag + "cost"][b, :n]
        assert ref.min() >= 1.0 and ref.max() <= 179.0
        assert np.array_equal(g[tag + "tol"][b, :n], [XH.pair_tolerance(a) for a in ref])
        assert (np.abs(cost[rows, cols] - ref) <= g[tag + "tol"][b, :n]).all()
