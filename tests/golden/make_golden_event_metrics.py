#!/usr/bin/env python3
"""Generate tests/golden/event_metrics.npz by IMPORTING THE REFERENCE's metrics.py, Dcase21_metrics.py and
utility_functions.py and calling them on the cases of event_metrics_cases.py.

Needs a checkout of the reference (read-only), whose directory SELD_REFERENCE names:

    SELD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_event_metrics.py

The reference's metrics.py configures task-1 speech packages at import time; absent ones get inert stand-ins (the recipe
of make_golden.py), and their names are recorded in `meta`.

Per case, under `<name>.`:
  lsd, sed     TP, FP, FN of location_sensitive_detection / sed_score_computation, summed over the recordings (absent for
               a case whose detection part is a KeyError, which is asserted here)
  dcase        _TP _FP _FN _S _D _I _Nref _DE_TP _DE_FP _DE_FN of one SELDMetrics after segment_labels +
               update_seld_scores on every recording;  total_DE its _total_DE;  scores its compute_seld_scores()
  seg.*        for SEGMENT_CASES: segment_labels' result for the predictions of recording 0, flattened (flatten_segments)
and `host.*`: the host functions on host_function_inputs().

Two conditions keep a tie-break or a last bit from deciding a counter; a case that violates one is an error here (pick
another seed in the case table): no prediction/reference distance within 1e-9 of the spatial threshold and no track
average within 1e-9 of the DOA threshold; every association's best assignment leads the second best by more than 1e-9.
The numpy restatement of tests/event_metrics_helpers.py must agree with the reference on every case as well.
The archive is written with fixed timestamps, so that regenerating it gives the same bytes.
"""
import importlib
import importlib.machinery
import io
import json
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ["SELD_REFERENCE"])

from tests.event_metrics_helpers import score_case  # noqa: E402
from tests.golden.event_metrics_cases import (EVENT_METRIC_CASES, SEGMENT_CASES, decoded, frame_dict,  # noqa: E402
                                              host_function_inputs)


class _AbsentThing:
    def __getattr__(self, item):
        if item.startswith("__"):
            raise AttributeError(item)
        return _AbsentThing()

    def __call__(self, *a, **k):
        return _AbsentThing()


class _Absent(types.ModuleType):
    def __init__(self, name):
        super().__init__(name)
        self.__spec__ = importlib.machinery.ModuleSpec(name, None)
        self.__path__ = []

    def __getattr__(self, item):
        if item.startswith("__"):
            raise AttributeError(item)
        return _AbsentThing()


def import_reference(name, stubbed):
    while True:
        try:
            return importlib.import_module(name)
        except ImportError as e:
            if e.name is None or e.name in stubbed or len(stubbed) > 12:
                raise
            stubbed.append(e.name)
            sys.modules[e.name] = _Absent(e.name)


def flatten_segments(seg):
    """index (1 + N, 3) int64: [blocks, 0, 0] then [block, class, frames] per (block, class) in iteration order; keys: the
    frame keys of all of them in order; counts: events under each key; entries (M, 4): [x, y, z, event]."""
    index, keys, counts, entries = [[len(seg), 0, 0]], [], [], []
    for b in seg:
        for c in seg[b]:
            assert len(seg[b][c]) == 1
            ks, vals = seg[b][c][0]
            index.append([b, c, len(ks)])
            keys += ks
            counts += [len(v) for v in vals]
            entries += [e for v in vals for e in v]
    return (np.asarray(index, dtype=np.int64), np.asarray(keys, dtype=np.int64), np.asarray(counts, dtype=np.int64),
            np.asarray(entries, dtype=np.float64).reshape(-1, 4))


def main():
    stubbed = []
    RM = import_reference("metrics", stubbed)
    RD = import_reference("Dcase21_metrics", stubbed)
    RUF = import_reference("utility_functions", stubbed)
    out = {}
    # the (k) builders restate gen_submission_list_task2: check them against it
    for seed, density in ((50, 0.05), (1050, 0.05), (60, 0.30), (1060, 0.30)):
        lists, dense = decoded(seed, 20, 100, density)
        for rec, (sed, doa) in zip(lists, dense):
            ref = RUF.gen_submission_list_task2(sed, doa, max_loc_value=2., num_frames=100)[0]
            assert ref.reshape(-1, 5).tobytes() == rec.tobytes(), ("decoded", seed)
    for c in EVENT_METRIC_CASES:
        name = c["name"] + "."
        margins = dict(spatial=np.inf, doa=np.inf, assignment=np.inf)
        mine = score_case(c, margins)
        assert min(margins.values()) > 1e-9, (c["name"], margins)
        em = RD.SELDMetrics(doa_threshold=c["doa_threshold"], nb_classes=c["nb_classes"])
        lsd, sed = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64)
        for p, t in zip(c["pred"], c["true"]):
            pa, ta = (r if r.shape[0] else np.array([]) for r in (p, t))
            if c["lsd"]:
                lsd += RM.location_sensitive_detection(pa, ta, c["n_frames"], c["spatial_threshold"])[:3]
                try:
                    sed += RM.sed_score_computation(pa, ta, c["n_frames"], c["spatial_threshold"])[:3]
                except ZeroDivisionError:       # raised after the counting: take the counters from the class-only restatement
                    assert t.shape[0] == 0 or p.shape[0] == 0
                    sed += np.asarray(score_case(dict(c, pred=[p], true=[t]))["sed"])
            else:
                try:
                    RM.location_sensitive_detection(pa, ta, c["n_frames"], c["spatial_threshold"])
                    raise AssertionError("expected KeyError")
                except KeyError:
                    pass
            em.update_seld_scores(RD.segment_labels(frame_dict(p), c["n_frames"], c["fpb"]),
                                  RD.segment_labels(frame_dict(t), c["n_frames"], c["fpb"]))
        dc = [int(v) for v in (em._TP, em._FP, em._FN, em._S, em._D, em._I, em._Nref, em._DE_TP, em._DE_FP, em._DE_FN)]
        scores = [float(v) for v in em.compute_seld_scores()]
        if c["lsd"]:
            out[name + "lsd"], out[name + "sed"] = lsd, sed
            assert mine["lsd"] == lsd.tolist() and mine["sed"] == sed.tolist(), (c["name"], mine, lsd, sed)
        out[name + "dcase"] = np.asarray(dc, dtype=np.int64)
        out[name + "total_DE"] = np.asarray([float(em._total_DE)])
        out[name + "scores"] = np.asarray(scores)
        assert mine["dcase"] == dc, (c["name"], mine["dcase"], dc)
        assert abs(mine["total_DE"] - float(em._total_DE)) <= 1e-12 * max(1.0, abs(float(em._total_DE))), c["name"]
        assert np.allclose(mine["scores"], scores, rtol=1e-12, atol=1e-12), c["name"]
        if c["name"] in SEGMENT_CASES:
            for k, a in zip(("index", "keys", "counts", "entries"),
                            flatten_segments(RD.segment_labels(frame_dict(c["pred"][0]), c["n_frames"], c["fpb"]))):
                out[name + "seg." + k] = a
        print(f"{c['name']:20s} lsd {lsd.tolist()} sed {sed.tolist()} dcase {dc} DE {float(em._total_DE):.6f} "
              f"margins {margins['spatial']:.2e} {margins['doa']:.2e} {margins['assignment']:.2e}")
    cart, sph, errs = host_function_inputs()
    out["host.cartesian"] = RD.distance_between_cartesian_coordinates(*cart.T)
    out["host.spherical"] = RD.distance_between_spherical_coordinates_rad(*sph.T)
    out["host.early_stopping"] = np.asarray([RD.early_stopping_metric(e[:2], e[2:]) for e in errs])
    out["meta"] = np.asarray(json.dumps(dict(numpy=np.__version__, stand_ins=stubbed,
                                             reference="AuroraEchos/Sound-Event-Localization-and-Detection @ 2025-02-11"),
                                        sort_keys=True))
    path = os.path.join(HERE, "event_metrics.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(out[k], order="C"), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                       compress_type=zipfile.ZIP_DEFLATED)
    print("wrote event_metrics", len(out), "arrays", os.path.getsize(path), "bytes; stand-ins:", stubbed)


if __name__ == "__main__":
    main()
