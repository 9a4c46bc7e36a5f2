#!/usr/bin/env python3
"""Generate tests/golden/labels.npz by IMPORTING THE REFERENCE's utility_functions and calling its csv_to_matrix_task2,
segment_task2 and segment_waveforms.

Needs a checkout of the reference (read-only), whose directory SELD_REFERENCE names, and pandas:

    SELD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_labels.py

The reference's module imports librosa, which it does not use for these functions; where the import fails an empty
stand-in module is registered (the recipe of make_golden_decode.py) and its name is recorded in `meta`.

Per case of ENCODE_CASES the fixture stores, under `<name>.`:
  csv        the label file's text as bytes (uint8); `class_names` (one array for all cases) the class-name list
  raised     the name of the exception csv_to_matrix_task2 raised, "" when it returned
  matrix     what it returned: (frames, 4 * 14 * 3) float64, or (frames, 4 * 14) with no_overlaps (absent when it raised)
  first, last   per event, the first and last frame the reference fills: read off the matrix it returns for a label
             file that holds this event alone (int64)
  cls, xyz   per event, the class id and the position as pandas parsed it (int64, float64 (E, 3))
Per case of SEGMENT_CASES:
  raised     as above
  count      number of chunks; X.<i>, Y.<i> the chunks exactly as returned, dtype included (absent when it raised)
The archive is written with fixed timestamps, so that regenerating it gives the same bytes.
"""
import importlib
import importlib.machinery
import io
import json
import os
import sys
import tempfile
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ["SELD_REFERENCE"])

from tests.golden.labels_cases import (CLASS_NAMES, CSV_HEADER, ENCODE_CASES, SEGMENT_CASES, class_dict, encode_csv,  # noqa: E402
                                       segment_inputs)


def import_reference():
    stubbed = []
    while True:
        try:
            return importlib.import_module("utility_functions"), stubbed
        except ModuleNotFoundError as e:
            if e.name is None or e.name in stubbed or len(stubbed) > 4:
                raise
            stubbed.append(e.name)
            sys.modules[e.name] = types.ModuleType(e.name)
            sys.modules[e.name].__spec__ = importlib.machinery.ModuleSpec(e.name, None)


def call(fn, *args, **kw):
    try:
        return fn(*args, **kw), ""
    except Exception as e:                      # noqa: BLE001 -- the name is what the fixture records
        return None, type(e).__name__


def main():
    import pandas as pd
    RUF, stubbed = import_reference()
    out = {"class_names": np.asarray(CLASS_NAMES)}
    cd = class_dict()
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "labels.csv")

    def matrix_of(text, c, no_overlaps):
        with open(path, "w") as f:
            f.write(text)
        return call(RUF.csv_to_matrix_task2, path, cd, dur=c["dur"], step=c["step"], max_loc_value=c["max_loc"],
                    no_overlaps=no_overlaps)

    for c in ENCODE_CASES:
        name = c["name"] + "."
        text = encode_csv(c)
        m, raised = matrix_of(text, c, c["no_overlaps"])
        assert raised == c["raises"], (c["name"], raised)          # in particular: no non-overflow case raises
        out[name + "csv"] = np.frombuffer(text.encode(), dtype=np.uint8)
        out[name + "raised"] = np.asarray(raised)
        if m is not None:
            assert m.dtype == np.float64
            out[name + "matrix"] = m
        lines = text.splitlines()[1:]
        first, last = [], []
        for ln in lines:
            one, r1 = matrix_of(CSV_HEADER + "\n" + ln + "\n", c, True)
            assert r1 == "", (c["name"], ln, r1)
            active = np.nonzero(one[:, :len(CLASS_NAMES)].sum(1))[0]
            assert active.size and np.array_equal(active, np.arange(active[0], active[-1] + 1)), (c["name"], ln)
            first.append(active[0])
            last.append(active[-1])
        with open(path, "w") as f:
            f.write(text)
        df = pd.read_csv(path)
        out[name + "first"] = np.asarray(first, dtype=np.int64)
        out[name + "last"] = np.asarray(last, dtype=np.int64)
        out[name + "cls"] = np.asarray([cd[k] for k in df["Class"]], dtype=np.int64)
        out[name + "xyz"] = df[["X", "Y", "Z"]].to_numpy(dtype=np.float64).reshape(len(lines), 3)
        cells = 0 if m is None else int(m[:, :m.shape[1] // 4].sum())
        print(f"{c['name']:20s} events {len(lines):3d} raised {raised or '-':10s} active cells {cells}")

    for c in SEGMENT_CASES:
        name = c["name"] + "."
        p, t = segment_inputs(c)
        res, raised = call(getattr(RUF, c["fn"]), p, t, **c["kw"])
        assert raised == c["raises"], (c["name"], raised)
        out[name + "raised"] = np.asarray(raised)
        if res is not None:
            X, Y = res
            assert len(X) == len(Y)
            out[name + "count"] = np.asarray(len(X))
            for i, (x, y) in enumerate(zip(X, Y)):
                out[f"{name}X.{i}"] = x
                out[f"{name}Y.{i}"] = y
            ragged = len({y.shape for y in Y}) > 1
            assert ragged == c["ragged"], (c["name"], [y.shape for y in Y])
            print(f"{c['name']:20s} chunks {len(X):3d} X {X[0].shape} {X[0].dtype}/{X[-1].dtype} "
                  f"Y {Y[0].shape} {Y[0].dtype}/{Y[-1].dtype} ragged {ragged}")
        else:
            print(f"{c['name']:20s} raised {raised}")
    out["meta"] = np.asarray(json.dumps(dict(numpy=np.__version__, pandas=pd.__version__, stand_ins=stubbed,
                                             encode_cases=[c["name"] for c in ENCODE_CASES],
                                             segment_cases=[c["name"] for c in SEGMENT_CASES],
                                             reference="AuroraEchos/Sound-Event-Localization-and-Detection @ 2025-02-11"),
                                        sort_keys=True))
    os.remove(path)
    os.rmdir(tmp)
    dst = os.path.join(HERE, "labels.npz")
    with zipfile.ZipFile(dst, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(out[k], order="C"), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                       compress_type=zipfile.ZIP_DEFLATED)
    print("wrote labels", len(out), "arrays", os.path.getsize(dst), "bytes; stand-ins:", stubbed)


if __name__ == "__main__":
    main()
