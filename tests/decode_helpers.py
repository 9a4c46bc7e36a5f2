"""Helpers shared by the event-decoding tests (tests/test_decode_host.py, tests/test_gpu_decode.py)."""
import numpy as np

from oracle import seld_oracle as O


def oracle_rows(sed, doa, max_loc_value, num_classes, max_overlaps):
    """(rows (E, 5) float64, event (E,)) from oracle.decode_events: frame-major, slot order."""
    active, xyz = O.decode_events(sed, doa, max_loc_value, num_classes, max_overlaps)
    f, c, e = np.nonzero(active)                                  # row-major order = frame, class, event
    rows = np.concatenate([f[:, None].astype(np.float64), c[:, None].astype(np.float64), xyz[f, c, e]], axis=1)
    return rows.reshape(-1, 5), e.astype(np.int32)


def fixture_dict(g, name):
    """The reference's dict of a case, rebuilt from its flattened form (Python int / float entries)."""
    entries = g[name + ".entries"]
    d, at = {}, 0
    for k, cnt in zip(g[name + ".keys"].tolist(), g[name + ".counts"].tolist()):
        d[k] = [[int(r[0]), float(r[1]), float(r[2]), float(r[3]), int(r[4])] for r in entries[at:at + cnt]]
        at += cnt
    assert at == entries.shape[0]
    return d
