"""Scoring event lists on the device (csrc/event_metrics.hip, hip_ops.score_events, the metrics and Dcase21_metrics drop-in
modules) against what the reference recorded in tests/golden/event_metrics.npz and against the fused dense path."""
import numpy as np
import pytest
import torch

from tests import event_metrics_helpers as EH
from tests.golden.cases import metric_inputs
from tests.golden.event_metrics_cases import CASE_IDS, EVENT_METRIC_CASES, frame_dict
from tests.helpers import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DCASE_ATTRS = ("_TP", "_FP", "_FN", "_S", "_D", "_I", "_Nref", "_DE_TP", "_DE_FP", "_DE_FN")


def _case(name):
    return EVENT_METRIC_CASES[CASE_IDS.index(name)]


def _device_lists(lists):
    """(rows, offsets) on the device, every recording ascending by frame (the wrapper's duty for score_events)."""
    rows = np.concatenate([EH.stable_by_frame(r) for r in lists])
    return torch.from_numpy(np.ascontiguousarray(rows)).to(DEV), torch.from_numpy(EH.offsets_of(lists)).to(DEV)


def _score(case, acc=None, select=slice(None), **kw):
    H = pkg().hip_ops
    acc = H.event_metrics_new(DEV) if acc is None else acc
    pr, po = _device_lists(case["pred"][select])
    tr, to = _device_lists(case["true"][select])
    H.score_events(acc, pr, po, tr, to, case["n_frames"], nb_classes=case["nb_classes"],
                   spatial_threshold=case["spatial_threshold"], doa_threshold=case["doa_threshold"],
                   frames_per_block=case["fpb"], **kw)
    return acc


def _close(a, b):
    return abs(a - b) <= 1e-12 * max(1.0, abs(b))


@pytest.mark.parametrize("case", EVENT_METRIC_CASES, ids=CASE_IDS)
def test_score_events_matches_reference(case, golden):
    """The 16 counters exact, total_de and the four scores to 1e-12."""
    H, T = pkg().hip_ops, pkg().train
    g, name = golden("event_metrics"), case["name"] + "."
    flags = torch.full((2,), -1, device=DEV, dtype=torch.int64)
    acc = _score(case, flags=flags)
    counters, total_de = acc[0].tolist(), float(acc[1].item())
    assert counters[3:13] == g[name + "dcase"].tolist()
    if case["lsd"]:
        assert counters[0:3] == g[name + "lsd"].tolist() and counters[13:16] == g[name + "sed"].tolist()
        assert flags.tolist() == [0, 0]
    else:
        beyond = sum(int((r[:, 0] >= case["n_frames"]).sum()) for r in case["pred"] + case["true"])
        assert flags.tolist() == [beyond, 0] and beyond > 0
        without = _case("g_without_27")          # rows beyond n_frames take no part in the detection counters
        assert counters[0:3] == g[without["name"] + ".lsd"].tolist()
        assert counters[13:16] == g[without["name"] + ".sed"].tolist()
    assert _close(total_de, float(g[name + "total_DE"][0]))
    D = pkg().Dcase21_metrics
    em = D.SELDMetrics(doa_threshold=case["doa_threshold"], nb_classes=case["nb_classes"])
    em._add(acc)
    assert np.allclose(em.compute_seld_scores(), g[name + "scores"], rtol=1e-12, atol=1e-12)
    if counters[9]:                                   # the 13 leading counters are train.py's, in its order
        assert len(T.test_results_from_counters(dict(zip(H.METRIC_COUNTERS, counters)), total_de)) == 16


@pytest.mark.parametrize("on_device", [False, True], ids=["numpy", "tensor"])
@pytest.mark.parametrize("case", EVENT_METRIC_CASES, ids=CASE_IDS)
def test_drop_in_functions(case, on_device, golden):
    """Every case, recording by recording as the reference is called, the counters summed.  The (l) cases are out of frame
    order: they go through the wrappers' sort."""
    M, D = pkg().metrics, pkg().Dcase21_metrics
    g, name = golden("event_metrics"), case["name"] + "."
    lsd, sed = [0, 0, 0], [0, 0, 0]
    em = D.SELDMetrics(doa_threshold=case["doa_threshold"], nb_classes=case["nb_classes"])
    for p, t in zip(case["pred"], case["true"]):
        pa, ta = (r if r.shape[0] else np.array([]) for r in (p, t))
        if on_device:
            pa, ta = (torch.from_numpy(np.asarray(r, dtype=np.float32 if case["name"].startswith("a_") else np.float64)).to(DEV)
                      .reshape(-1, 5) for r in (pa, ta))
        args = (pa, ta, case["n_frames"], case["spatial_threshold"])
        if not case["lsd"]:
            with pytest.raises(KeyError):
                M.location_sensitive_detection(*args)
            with pytest.raises(KeyError):
                M.sed_score_computation(*args)
        else:
            TP, FP, FN, F = M.location_sensitive_detection(*args)
            assert all(type(v) is int for v in (TP, FP, FN)) and F == EH.f_score(TP, FP, FN)
            lsd = [a + b for a, b in zip(lsd, (TP, FP, FN))]
            if t.shape[0] == 0:                       # a row list can be empty on the reference side: Nref == 0
                with pytest.raises(ZeroDivisionError):
                    M.sed_score_computation(*args)
                sed[1] += 2 * p.shape[0]              # what the reference counted before it divided
            else:
                TP, FP, FN, score = M.sed_score_computation(*args)
                assert score == np.mean([1 - EH.f_score(TP, FP, FN), (max(TP + FN, TP + FP) - TP) / (TP + FN + 0.0)])
                sed = [a + b for a, b in zip(sed, (TP, FP, FN))]
        if not on_device:
            em.update_seld_scores(D.segment_labels(frame_dict(p), case["n_frames"], case["fpb"]),
                                  D.segment_labels(frame_dict(t), case["n_frames"], case["fpb"]))
    if case["lsd"]:
        assert lsd == g[name + "lsd"].tolist() and sed == g[name + "sed"].tolist()
    if not on_device:
        assert [getattr(em, a) for a in DCASE_ATTRS] == g[name + "dcase"].tolist()
        assert _close(em._total_DE, float(g[name + "total_DE"][0]))
        assert np.allclose(em.compute_seld_scores(), g[name + "scores"], rtol=1e-12, atol=1e-12)


def test_dictionaries_and_rows_leave_identical_attributes():
    D = pkg().Dcase21_metrics
    case = _case("k_decoded_30")
    a, b = D.SELDMetrics(), D.SELDMetrics()
    for p, t in zip(case["pred"][:4], case["true"][:4]):
        a.update_seld_scores(D.segment_labels(frame_dict(p), 100), D.segment_labels(frame_dict(t), 100))
    pr, po = _device_lists(case["pred"][:4])
    tr, to = _device_lists(case["true"][:4])
    b.update_from_events(pr, po, tr, to, 100)
    assert [getattr(a, k) for k in DCASE_ATTRS] == [getattr(b, k) for k in DCASE_ATTRS] and a._Nref > 0
    assert _close(a._total_DE, b._total_DE)


def _write_csv(path, rec, names=None):
    with open(path, "w") as f:
        for fr, c, x, y, z in rec.tolist():
            f.write(f"{int(fr)},{names[int(c)] if names else int(c)},{x!r},{y!r},{z!r}\n")


def test_from_csv_numeric_and_named_classes(tmp_path, golden):
    M = pkg().metrics
    case = _case("h_overlaps")
    g = golden("event_metrics")
    names = {v: k for k, v in M.sound_classes_dict_task2.items()}
    for tag, table in (("numeric", None), ("named", names)):
        pp, tp = tmp_path / f"pred_{tag}.csv", tmp_path / f"true_{tag}.csv"
        _write_csv(pp, case["pred"][0], table)
        _write_csv(tp, case["true"][0], table)
        out = M.location_sensitive_detection(str(pp), str(tp), case["n_frames"], case["spatial_threshold"], from_csv=True)
        assert list(out[:3]) == g["h_overlaps.lsd"].tolist()
        out = M.sed_score_computation(str(pp), str(tp), case["n_frames"], from_csv=True)
        assert list(out[:3]) == g["h_overlaps.sed"].tolist()
    # files whose rows are out of frame order (a recording of an (l) case) count as the ordered lists of (k) do
    shuffled, ordered = _case("l_shuffled_30"), _case("k_decoded_30")
    for tag, table in (("numeric", None), ("named", names)):
        pp, tp = tmp_path / f"pred_l_{tag}.csv", tmp_path / f"true_l_{tag}.csv"
        _write_csv(pp, shuffled["pred"][3], table)
        _write_csv(tp, shuffled["true"][3], table)
        assert np.any(np.diff(shuffled["pred"][3][:, 0]) < 0) and np.any(np.diff(shuffled["true"][3][:, 0]) < 0)
        want = EH.detection_counts(ordered["pred"][3], ordered["true"][3], 100, 2.0)
        assert list(M.location_sensitive_detection(str(pp), str(tp), 100, 2.0, from_csv=True)[:3]) == want[0]
        assert list(M.sed_score_computation(str(pp), str(tp), 100, 2.0, from_csv=True)[:3]) == want[1]


def test_compute_seld_metrics_is_one_call_and_sums_the_files(tmp_path, capsys):
    M, C = pkg().metrics, pkg().hip_ops._core
    case = _case("k_decoded_05")
    (tmp_path / "pred").mkdir()
    (tmp_path / "truth").mkdir()
    TP = FP = FN = 0
    for k in range(6):
        _write_csv(tmp_path / "pred" / f"rec{k}.csv", case["pred"][k])
        _write_csv(tmp_path / "truth" / f"rec{k}.csv", case["true"][k])
        tp, fp, fn, _ = M.location_sensitive_detection(case["pred"][k], case["true"][k], 100, 2.0)
        TP, FP, FN = TP + tp, FP + fp, FN + fn
    C.kernel_timer.reset()
    C.kernel_timer.active = True
    try:
        F = M.compute_seld_metrics(str(tmp_path / "pred"), str(tmp_path / "truth"), 100, 2.0)
        torch.cuda.synchronize()
        calls = C.kernel_timer.summary()
    finally:
        C.kernel_timer.active = False
        C.kernel_timer.reset()
    assert calls["event_metrics_kernel"]["calls"] == 1
    eps = np.finfo(float).eps
    precision, recall = TP / (TP + FP + eps), TP / (TP + FN + eps)
    assert F == (2 * precision * recall) / (precision + recall + eps) and TP > 0
    assert "F score: " in capsys.readouterr().out


def test_consistent_with_the_fused_dense_path():
    """score_events on decode_events rows reproduces metrics_accumulate on the dense tensors they were decoded from."""
    H = pkg().hip_ops
    sed, doa, target = (torch.from_numpy(a).to(DEV) for a in metric_inputs(6, 100, 31, "mixed"))
    dense = H.metrics_new(DEV)
    H.metrics_accumulate(dense, sed, doa, target, 100)
    pr, _, po = H.decode_events(sed, doa)
    tr, _, to = H.decode_events(target[..., :42].contiguous(), target[..., 42:].contiguous())
    acc = H.score_events(H.event_metrics_new(DEV), pr, po, tr, to, 100)
    assert acc[0][:13].tolist() == dense[0].tolist() and int(dense[0][9]) > 0 and int(dense[0][0]) > 0
    assert _close(float(acc[1]), float(dense[1]))


def test_linearity():
    case = _case("k_decoded_30")
    whole = _score(case)
    halves = _score(case, select=slice(0, 10))
    _score(case, acc=halves, select=slice(10, 20))
    assert torch.equal(whole[0], halves[0]) and _close(float(halves[1]), float(whole[1]))


def test_sort_events_orders_shuffled_lists():
    H = pkg().hip_ops
    case, ref = _case("l_shuffled_05"), _case("k_decoded_05")
    rows = torch.from_numpy(np.concatenate(case["pred"])).to(DEV)
    offs = torch.from_numpy(EH.offsets_of(case["pred"])).to(DEV)
    assert torch.equal(H.sort_events(rows, offs).cpu(), torch.from_numpy(np.concatenate(ref["pred"])))


def test_refusals_leave_the_accumulators_untouched():
    H, L = pkg().hip_ops, pkg()._lib
    case = _case("h_overlaps")
    acc = _score(case)
    before = (acc[0].clone(), acc[1].clone())
    pr, po = _device_lists(case["pred"])
    tr, to = _device_lists(case["true"])

    def unchanged():
        torch.cuda.synchronize()
        return torch.equal(acc[0], before[0]) and acc[1].view(torch.int64).equal(before[1].view(torch.int64))

    four = torch.tensor([[3., 2., 1., 0., 0.], [3., 2., 0., 1., 0.], [3., 5., 0., 1., 0.], [3., 2., 0., 0., 1.], [3., 2., 1., 1., 0.]],
                        device=DEV, dtype=torch.float64)
    o4 = torch.tensor([0, 5], device=DEV)
    with pytest.raises(L.SeldHipError, match="3"):
        H.score_events(acc, four, o4, tr, to, 30)
    assert unchanged()
    with pytest.raises(L.SeldHipError, match="3"):
        H.score_events(acc, pr, po, four, o4, 30)
    assert unchanged()
    flags = torch.zeros(2, device=DEV, dtype=torch.int64)
    H.score_events(acc, four, o4, tr, to, 30, flags=flags)             # the caller reads the flags: nothing raised, nothing added
    assert flags.tolist() == [0, 1] and unchanged()
    H.score_events(H.event_metrics_new(DEV), four, o4, tr, to, 30, nb_classes=2)      # class 2 is not scored: no refusal
    for bad in (lambda: H.score_events(acc, pr, po, tr, to, 30, nb_classes=65),
                lambda: H.score_events(acc, pr, po, tr, to, 30, frames_per_block=0),
                lambda: H.score_events(acc, pr.float(), po, tr, to, 30),
                lambda: H.score_events(acc, pr, po.int(), tr, to, 30),
                lambda: H.score_events(acc, pr.cpu(), po, tr, to, 30),
                lambda: H.score_events(acc, pr, po, tr, to.cpu(), 30),
                lambda: H.score_events(acc, pr, po, tr, torch.tensor([0, 1, tr.shape[0]], device=DEV), 30)):
        with pytest.raises(L.SeldHipError):
            bad()
        assert unchanged()
    M = pkg().metrics                                       # the detection has no limit on a frame's events of one class
    assert M.location_sensitive_detection(four.cpu().numpy(), four, 10)[:3] == (5, 0, 0)


def test_empty_lists_and_recordings():
    H = pkg().hip_ops
    none = torch.empty((0, 5), device=DEV, dtype=torch.float64)
    for R in (0, 1, 3):
        offs = torch.zeros(R + 1, device=DEV, dtype=torch.int64)
        acc = H.score_events(H.event_metrics_new(DEV), none, offs, none, offs, 50)
        assert int(acc[0].abs().sum()) == 0 and float(acc[1]) == 0.0
