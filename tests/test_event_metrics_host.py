"""Event-list scoring without a GPU: the numpy restatement of tests/event_metrics_helpers.py, the package's host functions
and segment_labels against what the reference recorded in tests/golden/event_metrics.npz."""
import numpy as np
import pytest

from tests import event_metrics_helpers as EH
from tests.golden.event_metrics_cases import (CASE_IDS, EVENT_METRIC_CASES, SEGMENT_CASES, frame_dict,
                                              host_function_inputs)
from tests.helpers import pkg


@pytest.mark.parametrize("case", EVENT_METRIC_CASES, ids=CASE_IDS)
def test_restatement_matches_reference(case, golden):
    """Counters exact, floats to 1e-12 (the figure tests/test_gpu_metrics.py uses for these quantities)."""
    g, name = golden("event_metrics"), case["name"] + "."
    mine = EH.score_case(case)
    if case["lsd"]:
        assert mine["lsd"] == g[name + "lsd"].tolist() and mine["sed"] == g[name + "sed"].tolist()
    else:
        assert name + "lsd" not in g
        with pytest.raises(KeyError):
            EH.detection_counts(case["pred"][0], case["true"][0], case["n_frames"], case["spatial_threshold"])
    assert mine["dcase"] == g[name + "dcase"].tolist()
    ref_de = float(g[name + "total_DE"][0])
    assert abs(mine["total_DE"] - ref_de) <= 1e-12 * max(1.0, abs(ref_de))
    assert np.allclose(mine["scores"], g[name + "scores"], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", SEGMENT_CASES)
def test_segment_labels_equals_reference_structure(name, golden):
    D = pkg().Dcase21_metrics
    g = golden("event_metrics")
    case = EVENT_METRIC_CASES[CASE_IDS.index(name)]
    ref = EH.rebuild_segments(*(g[f"{name}.seg.{k}"] for k in ("index", "keys", "counts", "entries")))
    got = D.segment_labels(frame_dict(case["pred"][0]), case["n_frames"], case["fpb"])
    assert got == ref
    assert list(got) == list(ref) and all(list(got[b]) == list(ref[b]) for b in ref)      # iteration order too


def test_host_functions_match_reference(golden):
    D = pkg().Dcase21_metrics
    g = golden("event_metrics")
    cart, sph, errs = host_function_inputs()
    assert np.allclose(D.distance_between_cartesian_coordinates(*cart.T), g["host.cartesian"], rtol=0, atol=1e-12)
    assert np.allclose(D.distance_between_spherical_coordinates_rad(*sph.T), g["host.spherical"], rtol=0, atol=1e-12)
    got = [D.early_stopping_metric(e[:2], e[2:]) for e in errs]
    assert np.allclose(got, g["host.early_stopping"], rtol=0, atol=1e-12)


def test_compute_seld_scores_and_names():
    """The drop-in surface: names and signatures of the reference, the scores' formulas from given counters."""
    import inspect
    M, D = pkg().metrics, pkg().Dcase21_metrics
    assert M.sound_classes_dict_task2["Writing"] == 13 and len(M.sound_classes_dict_task2) == 14
    assert list(inspect.signature(M.location_sensitive_detection).parameters) == \
        ["pred", "true", "n_frames", "spatial_threshold", "from_csv", "verbose"]
    assert list(inspect.signature(M.compute_seld_metrics).parameters) == \
        ["predicted_folder", "truth_folder", "n_frames", "spatial_threshold"]
    assert list(inspect.signature(D.segment_labels).parameters) == ["_pred_dict", "_max_frames", "_nb_label_frames_1s"]
    em = D.SELDMetrics()
    assert (em._spatial_T, em._nb_classes) == (20, 14)
    assert em.compute_seld_scores() == (0.0, 0.0, 180, 0.0)
    em._TP, em._FP, em._FN, em._S, em._D, em._I, em._Nref, em._DE_TP, em._DE_FN, em._total_DE = 5, 2, 3, 1, 2, 1, 8, 6, 2, 61.5
    assert np.allclose(em.compute_seld_scores(), EH.seld_scores([5, 2, 3, 1, 2, 1, 8, 6, 0, 2], 61.5), rtol=1e-15)


def test_abi_declares_the_entry_point():
    L = pkg()._lib
    with open(L.HEADER_PATH) as f:
        protos = L.prototypes(f.read())
    restype, argtypes = protos["seld_event_metrics_accumulate"]
    assert len(argtypes) == 16
