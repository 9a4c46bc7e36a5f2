"""The breakdown by recording and class on the device (hip_ops.score_events_by, hip_ops.metrics_accumulate_by; csrc/
event_metrics.hip, csrc/metrics.hip) against what the reference recorded in tests/golden/class_metrics.npz, against the numpy
restatement of tests/class_metrics_ref.py and against the plain calls; SELDMetrics(average='macro') and the test leg of
train.py on top of it.  Integers exact; total_de within total_de_tolerance of the fp64 evaluation, and the same bits from
run to run."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import class_metrics_ref as CR
from tests import event_metrics_helpers as EH
from tests.golden.class_metrics_cases import ALL_CASES, ALL_IDS, refused_lists
from tests.golden.event_metrics_cases import decoded
from tests.helpers import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_REF, _GOT = {}, {}


def _case(name):
    return ALL_CASES[ALL_IDS.index(name)]


def _ref(case):
    """The restatement's (counters, total_de, tolerance) of a case, computed once and left alone."""
    if case["name"] not in _REF:
        _REF[case["name"]] = CR.table(case)
    return _REF[case["name"]]


def _device_lists(lists, coords=3):
    rows = np.concatenate([EH.stable_by_frame(r) for r in lists]) if lists else np.zeros((0, 2 + coords))
    return torch.from_numpy(np.ascontiguousarray(rows)).to(DEV), torch.from_numpy(EH.offsets_of(lists)).to(DEV)


def _kw(case):
    return dict(nb_classes=case["nb_classes"], spatial_threshold=case["spatial_threshold"], doa_threshold=case["doa_threshold"],
                frames_per_block=case["fpb"], coords=case["coords"], max_tracks=case["max_tracks"])


def _by(case, select=slice(None), **kw):
    H = pkg().hip_ops
    pr, po = _device_lists(case["pred"][select], case["coords"])
    tr, to = _device_lists(case["true"][select], case["coords"])
    return H.score_events_by(pr, po, tr, to, case["n_frames"], **_kw(case), **kw)


def _got(case):
    """The device's (counters, total_de, flags) of a case as numpy, written into tables full of sevens; computed once."""
    if case["name"] not in _GOT:
        R, C = len(case["pred"]), case["nb_classes"]
        out = (torch.full((R, C + 2, 16), 7, device=DEV, dtype=torch.int64), torch.full((R, C + 2), 7., device=DEV, dtype=torch.float64))
        flags = torch.full((2,), -1, device=DEV, dtype=torch.int64)
        cnt, de = _by(case, flags=flags, out=out)
        assert cnt is out[0] and de is out[1]
        _GOT[case["name"]] = (cnt.cpu().numpy(), de.cpu().numpy(), flags.tolist())
    return _GOT[case["name"]]


def _dense_inputs(case_name):
    """(sed, doa, target) on the device for a k_decoded case: the dense tensors its rows were decoded from."""
    seed, density = {"k_decoded_05": (50, 0.05), "k_decoded_30": (60, 0.30)}[case_name]
    _, pred = decoded(seed, 20, 100, density)
    _, true = decoded(seed + 1000, 20, 100, density)
    sed, doa = (torch.from_numpy(np.stack([d[k] for d in pred])).to(DEV) for k in (0, 1))
    target = torch.from_numpy(np.stack([np.concatenate(d, 1) for d in true])).to(DEV)
    return sed, doa, target


@pytest.mark.parametrize("case", ALL_CASES, ids=ALL_IDS)
def test_score_events_by_matches_fixture_and_restatement(case, golden):
    g, name, C = golden("class_metrics"), case["name"] + ".", case["nb_classes"]
    cnt, de, flags = _got(case)
    ref_c, ref_de, tol = _ref(case)
    assert flags[1] == 0 and (flags[0] == 0) == case["lsd"]
    assert (cnt == ref_c).all(), np.argwhere(cnt != ref_c)[:5]
    known = g[name + "all"] >= 0
    assert (cnt[:, C + 1][known] == g[name + "all"][known]).all() and (cnt[:, :C, 3:13] == g[name + "cls"]).all()
    for got, want, t in ((de, ref_de, tol), (de[:, C + 1], g[name + "all_de"], tol[:, C + 1]), (de[:, :C], g[name + "cls_de"], tol[:, :C])):
        err = np.abs(got - want)
        print(case["name"], "total_de error", float(err.max()) if err.size else 0.0, "tolerance", float(t.max()) if t.size else 0.0)
        assert (err <= t).all()
    assert (de[:, C] == 0).all() and (cnt[:, C, 3:13] == 0).all()


@pytest.mark.parametrize("case", ALL_CASES, ids=ALL_IDS)
def test_rows_all_add_up_to_the_plain_call(case):
    H = pkg().hip_ops
    cnt, de, _ = _got(case)
    pr, po = _device_lists(case["pred"], case["coords"])
    tr, to = _device_lists(case["true"], case["coords"])
    acc = H.score_events(H.event_metrics_new(DEV), pr, po, tr, to, case["n_frames"], **_kw(case),
                         flags=torch.empty(2, device=DEV, dtype=torch.int64))
    assert cnt[:, -1].sum(0).tolist() == acc[0].tolist()
    total = float(acc[1].item())
    assert abs(float(de[:, -1].sum()) - total) <= 1e-12 * max(1.0, abs(total))
    tc, td = pkg().class_metrics.totals(cnt, de)
    assert tc[-1].tolist() == acc[0].tolist() and abs(float(td[-1]) - total) <= 1e-12 * max(1.0, abs(total))


@pytest.mark.parametrize("name", ["k_decoded_05", "k_decoded_30"])
def test_dense_path_matches_and_agrees_with_the_event_path(name, golden):
    H = pkg().hip_ops
    case, g = _case(name), golden("class_metrics")
    sed, doa, target = _dense_inputs(name)
    out = (torch.full((20, 16, 16), 7, device=DEV, dtype=torch.int64), torch.full((20, 16), 7., device=DEV, dtype=torch.float64))
    cnt, de = H.metrics_accumulate_by(sed, doa, target, 100, out=out)
    assert cnt is out[0]
    cnt, de = cnt.cpu().numpy(), de.cpu().numpy()
    ref_c, ref_de, tol = _ref(case)
    want = ref_c.copy()
    want[..., 13:16] = 0                                # the dense path has no class-only detection
    assert (want[:, 14] == 0).all() and (cnt == want).all(), np.argwhere(cnt != want)[:5]
    assert (cnt[:, 15, :13] == g[name + ".all"][:, :13]).all() and (cnt[:, :14, 3:13] == g[name + ".cls"]).all()
    assert (np.abs(de - ref_de) <= tol).all() and (np.abs(de[:, 15] - g[name + ".all_de"]) <= tol[:, 15]).all()
    # the event path on the rows decoded from the same tensors: the same table, total_de to the last bit or two
    ev_c, ev_de, _ = _got(case)
    assert (ev_c[..., :13] == cnt[..., :13]).all() and (np.abs(ev_de - de) <= 1e-12 * np.maximum(1.0, np.abs(de))).all()
    # rows "all" against the plain dense call, one launch and recording by recording slices of one table
    acc = H.metrics_accumulate(H.metrics_new(DEV), sed, doa, target, 100)
    assert cnt[:, 15, :13].sum(0).tolist() == acc[0].tolist()
    assert abs(float(de[:, 15].sum()) - float(acc[1])) <= 1e-12 * float(acc[1])
    parts = (torch.empty_like(out[0]), torch.empty_like(out[1]))
    H.metrics_accumulate_by(sed[:7], doa[:7], target[:7], 100, out=(parts[0][:7], parts[1][:7]))
    H.metrics_accumulate_by(sed[7:], doa[7:], target[7:], 100, out=(parts[0][7:], parts[1][7:]))
    assert torch.equal(parts[0], out[0]) and torch.equal(parts[1].view(torch.int64), out[1].view(torch.int64))


def test_two_runs_give_the_same_bits_and_slices_the_same_table():
    H = pkg().hip_ops
    for name in ("by_five", "k_decoded_30", "sph_general", "cart_dense"):
        case = _case(name)
        cnt, de, _ = _got(case)
        again_c, again_de = _by(case)
        assert np.array_equal(again_c.cpu().numpy(), cnt) and again_de.cpu().numpy().tobytes() == de.tobytes(), name
    # successive batches into successive slices of one table
    case = _case("by_five")
    cnt, de, _ = _got(case)
    whole = (torch.empty((5, 16, 16), device=DEV, dtype=torch.int64), torch.empty((5, 16), device=DEV, dtype=torch.float64))
    _by(case, select=slice(0, 2), out=(whole[0][:2], whole[1][:2]))
    _by(case, select=slice(2, 5), out=(whole[0][2:], whole[1][2:]))
    assert np.array_equal(whole[0].cpu().numpy(), cnt) and whole[1].cpu().numpy().tobytes() == de.tobytes()
    rev_c, rev_de, _ = _got(_case("by_five_reversed"))
    assert np.array_equal(rev_c, cnt[::-1]) and rev_de.tobytes() == de[::-1].tobytes()
    with pytest.raises(pkg()._lib.SeldHipError, match="out"):
        _by(case, out=(whole[0][:4], whole[1]))
    with pytest.raises(pkg()._lib.SeldHipError, match="out"):
        _by(case, out=(whole[0].int(), whole[1]))
    sed, doa, target = _dense_inputs("k_decoded_30")
    a = H.metrics_accumulate_by(sed, doa, target, 100)
    b = H.metrics_accumulate_by(sed, doa, target, 100)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))


def test_records_into_and_replays_from_a_graph():
    H = pkg().hip_ops
    case = _case("by_five")
    cnt, de, _ = _got(case)
    pr, po = _device_lists(case["pred"])
    tr, to = _device_lists(case["true"])
    sed, doa, target = (t[:3].contiguous() for t in _dense_inputs("k_decoded_05"))
    dense_want = H.metrics_accumulate_by(sed, doa, target, 100)
    out = (torch.zeros((5, 16, 16), device=DEV, dtype=torch.int64), torch.zeros((5, 16), device=DEV, dtype=torch.float64))
    dense_out = (torch.zeros((3, 16, 16), device=DEV, dtype=torch.int64), torch.zeros((3, 16), device=DEV, dtype=torch.float64))
    flags = torch.zeros(2, device=DEV, dtype=torch.int64)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        H.score_events_by(pr, po, tr, to, 30, flags=flags, out=out)
        H.metrics_accumulate_by(sed, doa, target, 100, out=dense_out)
    for t in out + dense_out:
        t.fill_(7)
    flags.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out[0].cpu().numpy(), cnt) and out[1].cpu().numpy().tobytes() == de.tobytes()
    assert flags.tolist() == [0, 0]
    assert torch.equal(dense_out[0], dense_want[0]) and torch.equal(dense_out[1].view(torch.int64), dense_want[1].view(torch.int64))


def test_a_refused_call_writes_zeros():
    H, L = pkg().hip_ops, pkg()._lib
    P, T = refused_lists()
    pr, po = _device_lists(P)
    tr, to = _device_lists(T)
    out = (torch.full((1, 16, 16), 7, device=DEV, dtype=torch.int64), torch.full((1, 16), 7., device=DEV, dtype=torch.float64))
    flags = torch.full((2,), -1, device=DEV, dtype=torch.int64)
    H.score_events_by(pr, po, tr, to, 30, flags=flags, out=out)
    assert flags.tolist() == [0, 1] and int(out[0].abs().sum()) == 0 and float(out[1].abs().sum()) == 0.0
    with pytest.raises(L.SeldHipError, match="3"):
        H.score_events_by(pr, po, tr, to, 30)
    taken = H.score_events_by(pr, po, tr, to, 30, max_tracks=4)         # four asked for: taken
    assert int(taken[0][0, 2, 9]) == 1 and int(taken[0][0, 15, 9]) == 2
    acc = H.score_events(H.event_metrics_new(DEV), pr, po, tr, to, 30, max_tracks=4)
    assert taken[0][0, 15].tolist() == acc[0].tolist()
    for bad in (lambda: H.score_events_by(pr, po, tr, to, 30, nb_classes=65), lambda: H.score_events_by(pr, po, tr, to, 30, coords=4),
                lambda: H.score_events_by(pr.cpu(), po, tr, to, 30), lambda: H.score_events_by(pr, po, tr, to, 30, max_tracks=9),
                lambda: H.score_events_by(pr, po, tr, to, 30, frames_per_block=0)):
        with pytest.raises(L.SeldHipError):
            bad()


def test_a_short_workspace_launches_nothing():
    H, L = pkg().hip_ops, pkg()._lib
    case = _case("by_five")
    pr, po = _device_lists(case["pred"])
    tr, to = _device_lists(case["true"])
    need = L.lib().seld_metrics_breakdown_workspace(5, 30, 14, 10)
    work = torch.empty(need, device=DEV, dtype=torch.uint8)
    out = (torch.full((5, 16, 16), 7, device=DEV, dtype=torch.int64), torch.full((5, 16), 7., device=DEV, dtype=torch.float64))
    flags = torch.full((2,), -1, device=DEV, dtype=torch.int64)

    def call(nbytes):
        return L.lib().seld_event_metrics_breakdown(L.ptr(pr), L.ptr(po), pr.shape[0], L.ptr(tr), L.ptr(to), tr.shape[0], 5, 30, 14, 10,
                                                    3, 3, 2.0, 20.0, L.ptr(out[0]), L.ptr(out[1]), L.ptr(work), nbytes, L.ptr(flags),
                                                    L.current_stream())
    assert call(need - 1) == -2                          # SELD_EWORKSPACE
    torch.cuda.synchronize()
    assert flags.tolist() == [-1, -1] and int((out[0] != 7).sum()) == 0 and int((out[1] != 7).sum()) == 0
    assert call(need) == 0
    cnt, de, _ = _got(case)
    assert np.array_equal(out[0].cpu().numpy(), cnt) and out[1].cpu().numpy().tobytes() == de.tobytes()
    sed, doa, target = _dense_inputs("k_decoded_05")
    dense_need = L.lib().seld_metrics_breakdown_workspace(20, 100, 14, 10)
    big = torch.empty(dense_need, device=DEV, dtype=torch.uint8)
    d_out = (torch.full((20, 16, 16), 7, device=DEV, dtype=torch.int64), torch.full((20, 16), 7., device=DEV, dtype=torch.float64))
    rc = L.lib().seld_metrics_breakdown(L.ptr(sed), L.ptr(doa), L.ptr(target), 20, 100, 100, 14, 3, 2.0, 2.0, 20.0, 10,
                                        L.ptr(d_out[0]), L.ptr(d_out[1]), L.ptr(big), dense_need - 1, L.current_stream())
    torch.cuda.synchronize()
    assert rc == -2 and int((d_out[0] != 7).sum()) == 0


def test_seld_metrics_macro():
    D, CM = pkg().Dcase21_metrics, pkg().class_metrics
    case = _case("by_five")
    ref_c, ref_de, tol = _ref(case)
    pr, po = _device_lists(case["pred"])
    tr, to = _device_lists(case["true"])
    micro, macro = D.SELDMetrics(nb_classes=14), D.SELDMetrics(nb_classes=14, average="macro")
    micro.update_from_events(pr, po, tr, to, 30)
    for lo, hi in ((0, 2), (2, 5)):                     # two updates: the table grows recording by recording
        sub = [_device_lists(side[lo:hi]) for side in (case["pred"], case["true"])]
        macro.update_from_events(sub[0][0], sub[0][1], sub[1][0], sub[1][1], 30)
    for attr in ("_TP", "_FP", "_FN", "_S", "_D", "_I", "_Nref", "_DE_TP", "_DE_FP", "_DE_FN"):
        assert getattr(macro, attr) == getattr(micro, attr), attr
    assert macro._total_DE == pytest.approx(micro._total_DE, rel=1e-12)
    cnt, de = macro.table()
    assert np.array_equal(cnt, ref_c) and (np.abs(de - ref_de) <= tol).all()
    want = CM.macro_scores(cnt, de)
    assert macro.compute_seld_scores() == (want["ER"], want["F"], want["LE"], want["LR"])
    close = CM.macro_scores(ref_c, ref_de)
    assert want["LE"] == pytest.approx(close["LE"], abs=float(tol.max())) and (want["ER"], want["F"]) == (close["ER"], close["F"])
    assert macro.compute_seld_scores() != pytest.approx(micro.compute_seld_scores(), rel=1e-6)
    assert macro.class_scores()["Nref"].tolist() == CM.class_scores(ref_c, ref_de)["Nref"].tolist()
    assert macro.jackknife()["leave_one_out"].shape == (5, 5)


def test_evaluate_test_with_class_report(tmp_path, capsys):
    from tests.golden.cases import metric_inputs
    from tests.test_gpu_ensemble import _model, _model_input
    T = pkg().train
    model = _model()
    x, xd = _model_input(160)
    target = torch.from_numpy(metric_inputs(2, 8, 43, "crowded")[2])
    loader = [(torch.from_numpy(x[:, :, :, :64].copy()), target)]
    flags = ["--TextArgs=none", "--class_overlaps=3", "--output_classes=14", "--results_path=" + str(tmp_path)]
    plain = T.evaluate_test(model, torch.device(DEV), loader, num_frames=8, args=T.parse_args(flags))
    capsys.readouterr()
    assert not os.path.exists(tmp_path / "class_report.json")
    report = T.evaluate_test(model, torch.device(DEV), loader, num_frames=8, args=T.parse_args(flags + ["--class_report=True"]))
    out = capsys.readouterr().out
    assert report[:8] == plain[:8] and report == pytest.approx(plain, rel=1e-12, abs=1e-12) and len(report) == 16
    assert "F score: " in out and "macro (" in out and "early stopping metric (micro)" in out
    with open(tmp_path / "class_report.json") as f:
        rep = json.load(f)
    assert rep["recordings"] == 2 and len(rep["classes"]) == 14 and rep["early_stopping_metric"] == report[11]
    assert sum(c["Nref"] for c in rep["classes"]) > 0
    macro = T.evaluate_test(model, torch.device(DEV), loader, num_frames=8, args=T.parse_args(flags + ["--metrics_average=macro"]))
    assert macro == report and "early stopping metric (macro)" in capsys.readouterr().out
    # whole recordings: the same switch in evaluate_recordings
    y = torch.from_numpy(metric_inputs(2, 20, 41, "crowded")[2]).to(DEV)
    common = dict(hop=32, table=None, epoch=3, batch=8, num_frames=20)
    args = T.parse_args(flags + ["--time_dim=64"])
    plain = T.evaluate_recordings(model, torch.device(DEV), xd, y, args, **common)
    report = T.evaluate_recordings(model, torch.device(DEV), xd, y, T.parse_args(flags + ["--time_dim=64", "--class_report=True"]),
                                   **common)
    assert report[:8] == plain[:8] and report == pytest.approx(plain, rel=1e-12, abs=1e-12)
    with open(tmp_path / "class_report.json") as f:
        assert json.load(f)["epoch"] == 3
