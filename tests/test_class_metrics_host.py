"""The breakdown by recording and class without a GPU: the numpy restatement (tests/class_metrics_ref.py) against what the
reference recorded in tests/golden/class_metrics.npz and against its sum invariant; the host arithmetic of class_metrics
against the formulas written out in numpy; what the new entry points answer to arguments they refuse (nothing is launched,
so made-up pointers do); the flags of train.py."""
import ctypes
import inspect
import sys
import types

import numpy as np
import pytest

from tests import class_metrics_ref as CR
from tests.golden.class_metrics_cases import ALL_CASES, ALL_IDS, SUB_A, SUB_B
from tests.helpers import pkg

EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -4
NULL, SOME = ctypes.c_void_p(0), ctypes.c_void_p(64)     # never dereferenced: every call here is refused before a launch
EPS = np.finfo(float).eps


@pytest.fixture(scope="module")
def tables():
    """name -> the restatement's (counters, total_de, tolerance), computed once."""
    memo = {}

    def get(case):
        if case["name"] not in memo:
            memo[case["name"]] = CR.table(case)
        return memo[case["name"]]
    return get


@pytest.mark.parametrize("case", ALL_CASES, ids=ALL_IDS)
def test_restatement_matches_the_reference_and_sums_up(case, golden, tables):
    g, name, C = golden("class_metrics"), case["name"] + ".", case["nb_classes"]
    cnt, de, tol = tables(case)
    R = len(case["pred"])
    assert cnt.shape == (R, C + 2, 16) and de.shape == tol.shape == (R, C + 2)
    ref_all = g[name + "all"]
    known = ref_all >= 0                                # -1: the reference records nothing there
    assert known[:, 3:13].all() and (cnt[:, C + 1][known] == ref_all[known]).all()
    assert (cnt[:, :C, 3:13] == g[name + "cls"]).all()
    assert (np.abs(de[:, C + 1] - g[name + "all_de"]) <= tol[:, C + 1]).all()
    assert (np.abs(de[:, :C] - g[name + "cls_de"]) <= tol[:, :C]).all()
    # rows 0 .. C sum to row "all", S, D, I apart; row "other" holds detection counters alone
    summed = list(CR.SUMMED)
    assert (cnt[:, :C + 1][..., summed].sum(1) == cnt[:, C + 1][..., summed]).all()
    assert (np.abs(de[:, :C + 1].sum(1) - de[:, C + 1]) <= tol[:, C + 1]).all()
    assert (cnt[:, C, 3:13] == 0).all() and (de[:, C] == 0).all()
    if case["coords"] == 2:
        assert (cnt[..., 0:3] == 0).all()


def test_new_cases_tell_the_definitions_apart(golden, tables):
    g = golden("class_metrics")
    five = next(c for c in ALL_CASES if c["name"] == "by_five")
    cnt, de, _ = tables(five)
    assert cnt[:, :14, 6].sum() != cnt[:, 15, 6].sum()                  # class-wise S against cross-class S
    assert cnt[3, SUB_A, 6:9].tolist() == [0, 1, 0] and cnt[3, SUB_B, 6:9].tolist() == [0, 0, 1]
    assert cnt[3, 15, 6:9].tolist() == [1, 0, 0]
    assert (cnt[0] == 0).all() and (cnt[1, 14, [0, 1, 2, 13, 14, 15]] != 0).any()       # the empty one; row "other"
    assert cnt[2, 6, 1] == -1 and cnt[2, 6, 14] == -1                     # a negative class FP
    rev = next(c for c in ALL_CASES if c["name"] == "by_five_reversed")
    rcnt, rde, _ = tables(rev)
    assert (rcnt == cnt[::-1]).all() and (rde == de[::-1]).all()
    assert (g["by_five_reversed.cls"] == g["by_five.cls"][::-1]).all()
    c64 = next(c for c in ALL_CASES if c["name"] == "by_64_classes")
    cnt64 = tables(c64)[0]
    assert cnt64[0, 63, 9] > 0 and cnt64[0, 64, 13] > 0 and (cnt64[1] == 0).all()


# ---- class_metrics: the formulas, written out ---------------------------------------------------------------------------------
def _hand_table():
    """(3, 4 + 2, 16) and (3, 6): class 1 has references but no matched track (DE_TP == 0), class 3 is absent from the
    reference (Nref == 0) but predicted, class 2 has a negative FP."""
    rng = np.random.RandomState(5)
    c = rng.randint(0, 9, size=(3, 6, 16)).astype(np.int64)
    d = rng.uniform(5, 60, size=(3, 6))
    c[:, 1, 10], d[:, 1] = 0, 0.0
    c[:, 3, 9] = 0
    c[:, 2, 1] = -1
    c[:, 4, 3:13], d[:, 4] = 0, 0.0
    c[:, 5], d[:, 5] = c[:, :5].sum(1), d[:, :5].sum(1)
    return c, d


def _direct_class_scores(c, d):
    e = sys.float_info.epsilon
    rows = []
    for k in range(c.shape[0] - 2):
        x = c[k].astype(float)
        row = {}
        for tag, (tp, fp, fn) in (("", x[0:3]), ("sed_", x[13:16])):
            p, r = tp / (tp + fp + e), tp / (tp + fn + e)
            row[tag + "precision"], row[tag + "recall"], row[tag + "f1"] = p, r, 2 * ((p * r) / (p + r + e))
        row["ER"] = (x[6] + x[7] + x[8]) / float(x[9] + EPS)
        row["F"] = x[3] / (EPS + x[3] + 0.5 * (x[4] + x[5]))
        row["LE"] = d[k] / float(x[10] + EPS) if x[10] else 180
        row["LR"] = x[10] / (EPS + x[10] + x[12])
        row["Nref"] = int(x[9])
        rows.append(row)
    return rows


def test_totals_and_class_scores():
    CM = pkg().class_metrics
    c, d = _hand_table()
    tc, td = CM.totals(c, d)
    assert tc.dtype == np.int64 and (tc == c.sum(0)).all() and np.array_equal(td, d.sum(0))
    assert all(np.array_equal(a, b) for a, b in zip(CM.totals(tc, td), (tc, td)))        # totals of totals
    got = CM.class_scores(c, d)
    want = _direct_class_scores(tc, td)
    assert set(got) == set(want[0])
    for k, row in enumerate(want):
        for key, v in row.items():
            assert got[key][k] == pytest.approx(v, rel=1e-15, abs=0), (k, key)
    assert got["LE"][1] == 180 and got["Nref"][3] == 0 and got["Nref"].dtype == np.int64
    with pytest.raises(ValueError, match="16"):
        CM.totals(c[..., :13], d)


@pytest.mark.parametrize("over", ["reference", "all"])
def test_macro_scores(over):
    CM = pkg().class_metrics
    c, d = _hand_table()
    rows = _direct_class_scores(c.sum(0), d.sum(0))
    keep = [r for r in rows if r["Nref"] > 0] if over == "reference" else rows
    assert len(keep) == (3 if over == "reference" else 4)
    got = CM.macro_scores(c, d, over=over)
    for key in ("ER", "F", "LE", "LR"):
        assert got[key] == pytest.approx(np.mean([r[key] for r in keep]), rel=1e-15)
    es = np.mean([got["ER"], 1 - got["F"], got["LE"] / 180, 1 - got["LR"]])
    assert got["early_stopping_metric"] == pytest.approx(es, rel=1e-15) and got["classes"] == len(keep)
    assert got["early_stopping_metric"] == pytest.approx(
        pkg().Dcase21_metrics.early_stopping_metric([got["ER"], got["F"]], [got["LE"], got["LR"]]), rel=1e-15)
    with pytest.raises(ValueError, match="over"):
        CM.macro_scores(c, d, over="classes")
    empty = CM.macro_scores(np.zeros((2, 6, 16), dtype=np.int64), np.zeros((2, 6)))
    assert (empty["ER"], empty["F"], empty["LE"], empty["LR"], empty["classes"]) == (0.0, 0.0, 180.0, 0.0, 0)


def test_jackknife():
    CM = pkg().class_metrics
    c, d = _hand_table()
    R = c.shape[0]
    score = lambda tc, td: np.array([CM.macro_scores(tc, td)["ER"], CM.macro_scores(tc, td, over="all")["LE"]])   # noqa: E731
    got = CM.jackknife(c, d, score)
    theta = score(c.sum(0), d.sum(0))
    loo = np.stack([score(c.sum(0) - c[r], d.sum(0) - d[r]) for r in range(R)])
    assert np.array_equal(got["estimate"], theta) and np.allclose(got["leave_one_out"], loo, rtol=1e-15, atol=0)
    assert np.allclose(got["bias"], (R - 1) * (loo.mean(0) - theta), rtol=1e-12, atol=1e-15)
    assert np.allclose(got["stderr"], np.sqrt((R - 1) / R * ((loo - loo.mean(0)) ** 2).sum(0)), rtol=1e-12, atol=0)
    assert (got["stderr"] > 0).all()
    assert CM.jackknife(c, d)["estimate"].shape == (5,)                 # the default score: the macro vector
    with pytest.raises(ValueError, match="two recordings"):
        CM.jackknife(c[:1], d[:1], score)
    with pytest.raises(ValueError, match="two recordings"):
        CM.jackknife(c.sum(0), d.sum(0), score)


# ---- the C ABI without a launch ---------------------------------------------------------------------------------------------
def _event(lib, pred_count=0, true_count=0, recordings=1, n_frames=30, nb_classes=14, fpb=10, coords=3, max_tracks=3,
           out=SOME, work=SOME, work_bytes=1 << 40, flags=SOME):
    return lib.seld_event_metrics_breakdown(NULL, NULL, pred_count, NULL, NULL, true_count, recordings, n_frames, nb_classes,
                                            fpb, coords, max_tracks, 2.0, 20.0, out, out, work, work_bytes, flags, NULL)


def _dense(lib, clips=1, frames=30, num_frames=30, classes=14, overlaps=3, fpb=10, data=SOME, out=SOME, work=SOME,
           work_bytes=1 << 40):
    return lib.seld_metrics_breakdown(data, data, data, clips, frames, num_frames, classes, overlaps, 2.0, 2.0, 20.0, fpb, out,
                                      out, work, work_bytes, NULL)


def test_workspace_query_and_a_short_workspace():
    lib = pkg()._lib.lib()
    q = lib.seld_metrics_breakdown_workspace
    assert q(5, 30, 14, 10) == 5 * 3 * 16 * 17 * 8 and q(150, 600, 14, 10) == 150 * 60 * 16 * 17 * 8
    assert q(1, 25, 0, 10) == 3 * 2 * 17 * 8 and q(2, 30, 64, 10) == 2 * 3 * 66 * 17 * 8 and q(0, 30, 14, 10) == 0
    assert q(1, 30, 65, 10) == 0 and q(1, 30, 14, 0) == 0 and q(-1, 30, 14, 10) == 0
    need = q(5, 30, 14, 10)
    # one byte short, or no workspace at all: refused before the flags are touched or anything is launched
    assert _event(lib, recordings=5, work_bytes=need - 1) == EWORKSPACE
    assert _event(lib, recordings=5, work=NULL, work_bytes=need) == EWORKSPACE
    assert _dense(lib, clips=5, work_bytes=need - 1) == EWORKSPACE
    assert _dense(lib, clips=5, work=NULL, work_bytes=need) == EWORKSPACE


def test_breakdown_refuses_where_the_plain_calls_do():
    lib = pkg()._lib.lib()
    for kw in (dict(coords=1), dict(coords=4), dict(max_tracks=0), dict(max_tracks=9), dict(nb_classes=65), dict(nb_classes=-1),
               dict(fpb=0), dict(recordings=-1), dict(pred_count=-1), dict(true_count=-1), dict(n_frames=-1), dict(pred_count=3),
               dict(true_count=3, coords=2, max_tracks=8), dict(out=NULL), dict(flags=NULL)):
        assert _event(lib, **kw) == EINVAL, kw
    assert _event(lib, pred_count=1 << 28) == EUNSUPPORTED and _event(lib, true_count=1 << 28, coords=2) == EUNSUPPORTED
    for kw in (dict(clips=-1), dict(frames=-1), dict(classes=0), dict(overlaps=0), dict(fpb=0), dict(out=NULL),
               dict(frames=31, num_frames=30), dict(data=NULL)):
        assert _dense(lib, **kw) == EINVAL, kw
    for kw in (dict(overlaps=4), dict(classes=22, overlaps=3), dict(fpb=65)):
        assert _dense(lib, **kw) == EUNSUPPORTED, kw
    assert _dense(lib, clips=0, data=NULL, work=NULL, work_bytes=0) == 0       # no recording: nothing to write


def test_header_and_signatures():
    L, H, D = pkg()._lib, pkg().hip_ops, pkg().Dcase21_metrics
    with open(L.HEADER_PATH) as f:
        protos = L.prototypes(f.read())
    ex, by = protos["seld_event_metrics_accumulate_ex"][1], protos["seld_event_metrics_breakdown"][1]
    assert by == ex[:16] + [ctypes.c_void_p, ctypes.c_size_t] + ex[16:]
    plain, dense = protos["seld_metrics_accumulate"][1], protos["seld_metrics_breakdown"][1]
    assert dense == plain[:14] + [ctypes.c_void_p, ctypes.c_size_t] + plain[14:]
    assert protos["seld_metrics_breakdown_workspace"] == (ctypes.c_size_t, [ctypes.c_int64] + [ctypes.c_int32] * 3)
    plain_sig, by_sig = inspect.signature(H.score_events).parameters, inspect.signature(H.score_events_by).parameters
    assert list(by_sig) == list(plain_sig)[1:] + ["out"] and by_sig["out"].default is None
    assert all(by_sig[k].default == plain_sig[k].default for k in list(plain_sig)[1:])
    dense_sig = inspect.signature(H.metrics_accumulate_by).parameters
    assert list(dense_sig) == list(inspect.signature(H.metrics_accumulate).parameters)[1:] + ["out"]
    assert "score_events_by" in H.event_metrics.__all__
    for name in ("totals", "class_scores", "macro_scores", "jackknife"):
        assert callable(getattr(pkg().class_metrics, name))
    em = D.SELDMetrics(nb_classes=5, average="macro")
    assert em._average == "macro" and D.SELDMetrics()._average == "micro" and D.SELDMetrics(30, 4, 8)._max_tracks == 8
    with pytest.raises(L.SeldHipError, match="average"):
        D.SELDMetrics(average="weighted")
    with pytest.raises(L.SeldHipError, match="update_from_events"):
        em.update_seld_scores({0: {}}, {0: {}})         # the dictionary form keeps no table
    with pytest.raises(L.SeldHipError, match="macro"):
        D.SELDMetrics().class_scores()
    c, d = em.table()
    assert c.shape == (0, 7, 16) and d.shape == (0, 7)


def test_train_flags():
    T = pkg().train
    args = T.parse_args([])
    assert args.class_report is False and args.metrics_average == "micro"
    assert T.class_report_from_args(args) == (False, "micro")
    assert T.class_report_from_args(T.parse_args(["--class_report", "True", "--metrics_average", "macro"])) == (True, "macro")
    assert T.class_report_from_args(None) == (False, "micro") and T.class_report_from_args(types.SimpleNamespace()) == (False, "micro")
    with pytest.raises(ValueError, match="metrics_average"):
        T.class_report_from_args(T.parse_args(["--metrics_average", "weighted"]))
    with pytest.raises(ValueError, match="class_report"):
        T.class_report_from_args(types.SimpleNamespace(class_report="yes"))
    bad = T.parse_args(["--metrics_average", "median", "--use_cuda", "False"])
    with pytest.raises(ValueError, match="metrics_average"):      # before the device is asked for (use_cuda False raises later)
        T.main(bad)


def test_class_report_from_a_table(tmp_path, capsys, tables):
    T, CM = pkg().train, pkg().class_metrics
    five = next(c for c in ALL_CASES if c["name"] == "by_five")
    cnt, de, _ = tables(five)
    results = T._results_from_table(cnt, de, 3)
    tc, td = CM.totals(cnt, de)
    assert results == T.test_results_from_counters(dict(zip(pkg().hip_ops.METRIC_COUNTERS, tc[-1].tolist())), float(td[-1]), 3)
    rep = T.class_report(cnt, de, results, epoch=3, average="macro", results_path=str(tmp_path / "res"))
    out = capsys.readouterr().out
    assert out.count("\n") == 1 + 14 + 2 and "macro (" in out and "+-" in out
    import json
    with open(tmp_path / "res" / "class_report.json") as f:
        assert json.load(f) == rep
    macro = CM.macro_scores(cnt, de)
    assert rep["early_stopping_metric"] == macro["early_stopping_metric"] and rep["macro"]["LE"] == macro["LE"]
    assert rep["micro"]["early_stopping_metric"] == results[11] and len(rep["classes"]) == 14 and rep["recordings"] == 5
    assert rep["macro_jackknife_stderr"]["ER"] == CM.jackknife(cnt, de)["stderr"][0]
    assert T.class_report(cnt, de, results, average="micro")["early_stopping_metric"] == results[11]
