#!/usr/bin/env python3
"""Generate tests/golden/decode.npz by IMPORTING THE REFERENCE's utility_functions and calling its
gen_submission_list_task2 and gen_submission_list_task2_OLD.

Needs a checkout of the reference (read-only), whose directory SELD_REFERENCE names:

    SELD_REFERENCE=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_decode.py

The reference's module imports librosa, which it does not use for these functions; where the import fails an empty
stand-in module is registered (the recipe of make_golden.py) and its name is recorded in `meta`.

Per case of DECODE_CASES the fixture stores, under `<name>.`:
  rows       what gen_submission_list_task2 returns first: (E, 5) float64, or (0,) without any event
  old_same   1 when gen_submission_list_task2_OLD returned the same shape, dtype and bytes (then it is not stored twice),
             else 0 and `rows_old` holds it
  keys, counts, entries   the returned dict, flattened since an .npz holds arrays: its keys in iteration order (int64),
             the number of entries under each key (int64), and all entries in order as (E, 5) float64
             [class, x, y, z, event]
  types      1 when every key and every class / event entry is a Python int and every coordinate a Python float
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

from tests.golden.decode_cases import DECODE_CASES, decode_inputs  # noqa: E402


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


def main():
    RUF, stubbed = import_reference()
    out = {}
    for c in DECODE_CASES:
        sed, doa = decode_inputs(c)
        kw = dict(max_loc_value=c["max_loc"], num_frames=c["T"], num_classes=c["classes"], max_overlaps=c["overlaps"])
        rows, d = RUF.gen_submission_list_task2(sed, doa, **kw)
        old = RUF.gen_submission_list_task2_OLD(sed, doa, **kw)
        assert rows.dtype == np.float64 and old.dtype == np.float64, (c["name"], rows.dtype, old.dtype)
        name = c["name"] + "."
        out[name + "rows"] = rows
        same = old.shape == rows.shape and old.tobytes() == rows.tobytes()
        out[name + "old_same"] = np.asarray(int(same))
        if not same:
            out[name + "rows_old"] = old
        entries = [e for v in d.values() for e in v]
        out[name + "keys"] = np.asarray(list(d.keys()), dtype=np.int64)
        out[name + "counts"] = np.asarray([len(v) for v in d.values()], dtype=np.int64)
        out[name + "entries"] = np.asarray(entries, dtype=np.float64).reshape(len(entries), 5)
        out[name + "types"] = np.asarray(int(all(type(k) is int for k in d) and all(
            [type(x) for x in e] == [int, float, float, float, int] for e in entries)))
        print(f"{c['name']:14s} rows {rows.shape} frames {len(d)} old_same {same}")
    out["meta"] = np.asarray(json.dumps(dict(numpy=np.__version__, stand_ins=stubbed,
                                             reference="AuroraEchos/Sound-Event-Localization-and-Detection @ 2025-02-11"),
                                        sort_keys=True))
    path = os.path.join(HERE, "decode.npz")
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(out[k], order="C"), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                       compress_type=zipfile.ZIP_DEFLATED)
    print("wrote decode", len(out), "arrays", os.path.getsize(path), "bytes; stand-ins:", stubbed)


if __name__ == "__main__":
    main()
