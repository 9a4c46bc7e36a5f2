"""What the label tests share: the fixture's cases unpacked, and plain-numpy statements of the two operations (the
specification the kernels are held to, themselves checked against the reference's fixture on the CPU)."""
import numpy as np

from tests.golden.labels_cases import CLASS_NAMES


def encode_events_host(g, name):
    """(first, last, cls, xyz) of an encode case as the fixture recorded them from the reference."""
    return tuple(g[f"{name}.{k}"] for k in ("first", "last", "cls", "xyz"))


def csv_times(text):
    """(start, end) columns of a label file's text as float64 arrays."""
    rows = [ln.split(",") for ln in text.splitlines()[1:]]
    return (np.asarray([float(r[1]) for r in rows], dtype=np.float64),
            np.asarray([float(r[2]) for r in rows], dtype=np.float64))


def encode_numpy(first, last, cls, xyz, frames, classes=14, overlaps=3, max_loc=2.0, no_overlaps=False):
    """The dense target of ONE recording and the number of overflowing (frame, class) cells: events in order, each
    taking the next free slot of its class in every frame it covers."""
    cl = np.zeros((frames, classes, overlaps))
    loc = np.zeros((frames, classes, overlaps, 3))
    count = np.zeros((frames, classes), dtype=np.int64)
    for a, b, c, p in zip(first, last, cls, xyz):
        for f in range(int(a), int(b) + 1):
            k = count[f, c]
            if k < overlaps:
                cl[f, c, k] = 1.0
                loc[f, c, k] = p
            count[f, c] += 1
    loc = loc / max_loc
    if no_overlaps:
        cl, loc = cl[:, :, :1], loc[:, :, :1]
    return np.concatenate((cl.reshape(frames, -1), loc.reshape(frames, -1)), 1), int((count > overlaps).sum())


def expected_rows(first, last, cls, xyz, overlaps=3):
    """[frame, class, x, y, z] rows and slot of every (event, covered frame), sorted by (frame, class, slot): what
    decoding the encoded target gives back."""
    taken = {}
    rows = []
    for a, b, c, p in zip(first, last, cls, xyz):
        for f in range(int(a), int(b) + 1):
            k = taken.get((f, int(c)), 0)
            taken[(f, int(c))] = k + 1
            assert k < overlaps
            rows.append((f, int(c), k, p[0], p[1], p[2]))
    rows.sort(key=lambda r: r[:3])
    return (np.asarray([[r[0], r[1], r[3], r[4], r[5]] for r in rows], dtype=np.float64).reshape(len(rows), 5),
            np.asarray([r[2] for r in rows], dtype=np.int32))


def segment_numpy(x, seg_len, hop, segments, time_first=False):
    """Zero-padded cut by plain slicing: (segments, ..., seg_len), or (segments, seg_len, ...) with time_first."""
    x = np.asarray(x)
    if time_first:
        out = np.zeros((segments, seg_len) + x.shape[1:], dtype=x.dtype)
        for s in range(segments):
            piece = x[s * hop:s * hop + seg_len]
            out[s, :piece.shape[0]] = piece
    else:
        out = np.zeros((segments,) + x.shape[:-1] + (seg_len,), dtype=x.dtype)
        for s in range(segments):
            piece = x[..., s * hop:s * hop + seg_len]
            out[s, ..., :piece.shape[-1]] = piece
    return out


def fixture_chunks(g, name):
    """(X, Y) lists of a segment case as the reference returned them."""
    n = int(g[name + ".count"])
    return [g[f"{name}.X.{i}"] for i in range(n)], [g[f"{name}.Y.{i}"] for i in range(n)]


def class_names(g):
    names = [str(s) for s in g["class_names"].tolist()]
    assert names == CLASS_NAMES
    return names
