"""Spherical rows, up to 8 events of one class in a frame and the association alone on the device (csrc/event_metrics.hip:
seld_event_metrics_accumulate_ex, seld_least_distance) against what the reference recorded in
tests/golden/event_metrics_ex.npz."""
import numpy as np
import pytest
import torch

from tests import event_metrics_helpers as EH
from tests.golden.event_metrics_cases import CASE_IDS, EVENT_METRIC_CASES
from tests.golden.event_metrics_ex_cases import EVENT_METRIC_EX_CASES, EX_CASE_IDS, assign_problems, frame_dict
from tests.helpers import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DCASE_ATTRS = ("_TP", "_FP", "_FN", "_S", "_D", "_I", "_Nref", "_DE_TP", "_DE_FP", "_DE_FN")


def _device_lists(lists):
    rows = np.concatenate([EH.stable_by_frame(r) for r in lists])
    return torch.from_numpy(np.ascontiguousarray(rows)).to(DEV), torch.from_numpy(EH.offsets_of(lists)).to(DEV)


def _score(case, acc=None, **kw):
    H = pkg().hip_ops
    acc = H.event_metrics_new(DEV) if acc is None else acc
    pr, po = _device_lists(case["pred"])
    tr, to = _device_lists(case["true"])
    kw.setdefault("coords", case.get("coords", 3))
    kw.setdefault("max_tracks", case.get("max_tracks", 3))
    H.score_events(acc, pr, po, tr, to, case["n_frames"], nb_classes=case["nb_classes"],
                   spatial_threshold=case["spatial_threshold"], doa_threshold=case["doa_threshold"],
                   frames_per_block=case["fpb"], **kw)
    return acc


def _close(a, b):
    return abs(a - b) <= 1e-12 * max(1.0, abs(b))


def _de_ok(case, g, got):
    """Cartesian: the 1e-12 of the existing tests; spherical (and the tie cases): the tolerance the generator stored."""
    ref = float(g[case["name"] + ".total_DE"][0])
    err = abs(got - ref)
    tol = float(g[case["name"] + ".total_DE_tol"][0])
    print(f"{case['name']}: total_DE {got!r} reference {ref!r} |difference| {err:.3e} stored tolerance {tol:.3e}")
    if case["coords"] == 3 and case["kind"] != "ties":
        return _close(got, ref)
    return err <= tol


@pytest.mark.parametrize("case", EVENT_METRIC_EX_CASES, ids=EX_CASE_IDS)
def test_score_events_matches_reference(case, golden):
    D = pkg().Dcase21_metrics
    g, name = golden("event_metrics_ex"), case["name"] + "."
    flags = torch.full((2,), -1, device=DEV, dtype=torch.int64)
    acc = _score(case, flags=flags)
    counters, total_de = acc[0].tolist(), float(acc[1].item())
    assert flags.tolist() == [0, 0]
    assert counters[3:13] == g[name + "dcase"].tolist()
    assert counters[13:16] == g[name + "sed"].tolist()
    assert counters[0:3] == (g[name + "lsd"].tolist() if case["coords"] == 3 else [0, 0, 0])
    assert _de_ok(case, g, total_de)
    em = D.SELDMetrics(doa_threshold=case["doa_threshold"], nb_classes=case["nb_classes"])
    em._add(acc)
    assert np.allclose(em.compute_seld_scores(), g[name + "scores"], rtol=1e-12, atol=1e-12)
    if case["coords"] == 2:                             # counters 0-2 are left alone, whatever they hold
        acc = H_new_filled()
        _score(case, acc=acc)
        assert acc[0][:3].tolist() == [7, 7, 7] and (acc[0][3:] - 7).tolist() == counters[3:]


def H_new_filled():
    acc = pkg().hip_ops.event_metrics_new(DEV)
    acc[0].fill_(7)
    return acc


@pytest.mark.parametrize("case", EVENT_METRIC_EX_CASES, ids=EX_CASE_IDS)
def test_update_seld_scores_on_dictionaries(case, golden):
    D = pkg().Dcase21_metrics
    g, name = golden("event_metrics_ex"), case["name"] + "."
    em = D.SELDMetrics(doa_threshold=case["doa_threshold"], nb_classes=case["nb_classes"], max_tracks=case["max_tracks"])
    rows = D.SELDMetrics(doa_threshold=case["doa_threshold"], nb_classes=case["nb_classes"], max_tracks=case["max_tracks"])
    for p, t in zip(case["pred"], case["true"]):
        em.update_seld_scores(D.segment_labels(frame_dict(p), case["n_frames"], case["fpb"]),
                              D.segment_labels(frame_dict(t), case["n_frames"], case["fpb"]))
    pr, po = _device_lists(case["pred"])
    tr, to = _device_lists(case["true"])
    rows.update_from_events(pr, po, tr, to, case["n_frames"], case["fpb"])         # takes the width from the rows
    for m in (em, rows):
        assert [getattr(m, a) for a in DCASE_ATTRS] == g[name + "dcase"].tolist()
        assert _de_ok(case, g, m._total_DE)
        assert np.allclose(m.compute_seld_scores(), g[name + "scores"], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("spherical", [False, True], ids=["cart", "sph"])
def test_assign_doas_matches_reference(spherical, golden):
    H, D = pkg().hip_ops, pkg().Dcase21_metrics
    g, tag = golden("event_metrics_ex"), "assign.sph." if spherical else "assign.cart."
    gt, pred, gn, qn = assign_problems(spherical)
    cost, row, col, pairs = (t.cpu().numpy() for t in H.assign_doas(*(torch.from_numpy(a).to(DEV) for a in (gt, pred, gn, qn)),
                                                                   spherical=spherical))
    assert pairs.tolist() == g[tag + "pairs"].tolist() == np.minimum(gn, qn).tolist()
    assert row.dtype == np.int32 and np.array_equal(row, g[tag + "row"]) and np.array_equal(col, g[tag + "col"])
    err = np.abs(cost - g[tag + "cost"])
    print(f"{tag} largest |cost - reference| / tolerance: {np.max(err[g[tag + 'tol'] > 0] / g[tag + 'tol'][g[tag + 'tol'] > 0]):.3f}")
    assert (err <= g[tag + "tol"]).all()                # padding: cost 0 against tolerance 0
    for b in range(0, 81, 1 if spherical else 4):       # the drop-in function, problem by problem
        c, r, cl = D.least_distance_between_gt_pred(gt[b, :gn[b]], pred[b, :qn[b]])
        n = int(pairs[b])
        assert c.shape == r.shape == cl.shape == (n,) and c.dtype == np.float64 and r.dtype.kind == cl.dtype.kind == "i"
        assert r.tolist() == g[tag + "row"][b, :n].tolist() and cl.tolist() == g[tag + "col"][b, :n].tolist()
        assert (np.abs(c - g[tag + "cost"][b, :n]) <= g[tag + "tol"][b, :n]).all()
    with pytest.raises(pkg()._lib.SeldHipError, match="8"):
        D.least_distance_between_gt_pred(np.zeros((9, gt.shape[2])), pred[80])


def test_small_cells_give_the_same_bits_under_every_entry():
    """h_overlaps (cells up to 3 x 3) through (3, 3), (3, 8) and the old entry point."""
    H, L = pkg().hip_ops, pkg()._lib
    case = EVENT_METRIC_CASES[CASE_IDS.index("h_overlaps")]
    a, b = _score(case, max_tracks=3), _score(case, max_tracks=8)
    old = H.event_metrics_new(DEV)
    pr, po = _device_lists(case["pred"])
    tr, to = _device_lists(case["true"])
    flags = torch.empty(2, device=DEV, dtype=torch.int64)
    L.check(L.lib().seld_event_metrics_accumulate(
        L.ptr(pr), L.ptr(po), pr.shape[0], L.ptr(tr), L.ptr(to), tr.shape[0], 1, case["n_frames"], case["nb_classes"],
        case["fpb"], case["spatial_threshold"], case["doa_threshold"], L.ptr(old[0]), L.ptr(old[1]), L.ptr(flags),
        L.current_stream()), "seld_event_metrics_accumulate")
    torch.cuda.synchronize()
    assert int(a[0][10]) > 0 and flags.tolist() == [0, 0]
    for other in (b, old):
        assert torch.equal(a[0], other[0]) and a[1].view(torch.int64).equal(other[1].view(torch.int64))


def _cell(n, frame=3., cls=2.):
    xyz = np.stack((np.cos(np.arange(n) * 0.7), np.sin(np.arange(n) * 0.7), 0.1 * np.arange(n)), 1)
    rows = np.concatenate((np.full((n, 1), frame), np.full((n, 1), cls), xyz), 1)
    return torch.from_numpy(rows).to(DEV), torch.tensor([0, n], device=DEV)


def test_refusals_leave_the_accumulators_untouched():
    H, L = pkg().hip_ops, pkg()._lib
    case = EVENT_METRIC_EX_CASES[EX_CASE_IDS.index("cart_tracks")]
    acc = _score(case)
    before = (acc[0].clone(), acc[1].clone())
    pr, po = _device_lists(case["pred"])
    tr, to = _device_lists(case["true"])

    def unchanged():
        torch.cuda.synchronize()
        return torch.equal(acc[0], before[0]) and acc[1].view(torch.int64).equal(before[1].view(torch.int64))

    nine, o9 = _cell(9)
    flags = torch.full((2,), -1, device=DEV, dtype=torch.int64)
    H.score_events(acc, nine, o9, tr, to, 20, nb_classes=4, max_tracks=8, flags=flags)
    assert flags.tolist() == [0, 1] and unchanged()
    with pytest.raises(L.SeldHipError, match="more than 8 events"):
        H.score_events(acc, tr, to, nine, o9, 20, nb_classes=4, max_tracks=8)
    assert unchanged()
    four, o4 = _cell(4)
    with pytest.raises(L.SeldHipError, match="more than 3 events"):      # the default is still 3
        H.score_events(acc, four, o4, tr, to, 20, nb_classes=4)
    assert unchanged()
    three, o3 = _cell(3)                                # (cart_tracks' own cells go up to 8: not a partner under 4)
    taken = H.score_events(H.event_metrics_new(DEV), four, o4, three, o3, 20, nb_classes=4, max_tracks=4)   # 4 asked for: taken
    assert taken[0][3:5].tolist() == [3, 1]             # three tracks matched at distance 0, the fourth a false positive
    with pytest.raises(L.SeldHipError, match="1 .* more than 4 events"):
        H.score_events(acc, nine[:5].contiguous(), torch.tensor([0, 5], device=DEV), four, o4, 20, nb_classes=4, max_tracks=4)
    assert unchanged()
    sph = torch.zeros((3, 4), device=DEV, dtype=torch.float64)
    o3 = torch.tensor([0, 3], device=DEV)
    for bad in (lambda: H.score_events(acc, pr, po, tr, to, 20, coords=4),
                lambda: H.score_events(acc, pr, po, tr, to, 20, coords=1),
                lambda: H.score_events(acc, pr, po, tr, to, 20, max_tracks=0),
                lambda: H.score_events(acc, pr, po, tr, to, 20, max_tracks=9),
                lambda: H.score_events(acc, pr, po, tr, to, 20, max_tracks=2.5),
                lambda: H.score_events(acc, pr, po, tr, to, 20, coords=2),            # five columns are not spherical rows
                lambda: H.score_events(acc, sph, o3, sph, o3, 20),                    # nor four Cartesian ones
                lambda: H.score_events(acc, sph, o3, tr, to, 20, coords=2),
                lambda: H.score_events(acc, sph.float(), o3, sph, o3, 20, coords=2),
                lambda: H.score_events(acc, sph.cpu(), o3, sph, o3, 20, coords=2),
                lambda: H.assign_doas(sph, sph, o3, o3),
                lambda: H.assign_doas(torch.zeros((2, 8, 3), device=DEV), torch.zeros((2, 8, 3), device=DEV),
                                      torch.zeros(2, device=DEV, dtype=torch.int32), torch.zeros(2, device=DEV, dtype=torch.int32))):
        with pytest.raises(L.SeldHipError):
            bad()
        assert unchanged()
    rc = L.lib().seld_event_metrics_accumulate_ex(L.ptr(pr), L.ptr(po), pr.shape[0], L.ptr(tr), L.ptr(to), tr.shape[0], 1, 20, 4,
                                                  10, 3, 9, 2.0, 20.0, L.ptr(acc[0]), L.ptr(acc[1]), L.ptr(flags),
                                                  L.current_stream())
    assert rc == -1 and unchanged()
    D = pkg().Dcase21_metrics
    em = D.SELDMetrics(nb_classes=4)
    mixed = {0: {1: [[[0], [[[10.0, 20.0, 0]]]]]}}
    cart = {0: {1: [[[0], [[[1.0, 0.0, 0.0, 0]]]]]}}
    with pytest.raises(L.SeldHipError, match="two and of three"):
        em.update_seld_scores(mixed, cart)
    with pytest.raises(L.SeldHipError):
        em.update_seld_scores({0: {1: [[[0], [[[1.0, 0]]]]]}}, cart)
    assert em._Nref == 0


def test_graph_capture_with_flags():
    H = pkg().hip_ops
    case = EVENT_METRIC_EX_CASES[EX_CASE_IDS.index("sph_tracks")]
    eager = _score(case)
    pr, po = _device_lists(case["pred"])
    tr, to = _device_lists(case["true"])
    acc = H.event_metrics_new(DEV)
    flags = torch.zeros(2, device=DEV, dtype=torch.int64)

    def call():
        H.score_events(acc, pr, po, tr, to, case["n_frames"], nb_classes=case["nb_classes"], coords=2, max_tracks=8, flags=flags)
    call()                                              # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    acc[0].zero_()
    acc[1].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert flags.tolist() == [0, 0] and torch.equal(acc[0], eager[0]) and int(acc[0][10]) > 0
    assert _close(float(acc[1]), float(eager[1]))
