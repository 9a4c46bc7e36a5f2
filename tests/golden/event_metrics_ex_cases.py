"""Case table of the extended event-list scoring: spherical rows [frame, class, azimuth, elevation] in degrees, up to 8
events of one class in a frame, and the association alone (least_distance_between_gt_pred).  Shared by the fixture
generator (make_golden_event_metrics_ex.py, runs against the reference) and the tests.  Pure data + seeded inputs
(decode_cases.uniform).

A scoring case is a dict: name, kind ("general", "degenerate" or "ties": which of the generator's conditions it is held
to), coords (3 or 2), max_tracks (what the device is asked for), n_frames, fpb, nb_classes, doa_threshold,
spatial_threshold, and `pred` / `true`, one (E, 2 + coords) float64 array per recording."""
import numpy as np

from tests.golden.decode_cases import uniform

# eight directions 45 degrees of azimuth apart, elevations alternating: the references of a cell are jittered copies
BASE = np.array([[-157.5 + 45.0 * k, 25.0 if k % 2 else -25.0] for k in range(8)])
TRACK_COUNTS = (1, 2, 4, 5, 8)


def empty(coords):
    return np.zeros((0, 2 + coords), dtype=np.float64)


def to_xyz(deg, radius=1.5):
    az, el = deg[:, 0] * np.pi / 180, deg[:, 1] * np.pi / 180
    return radius * np.stack((np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)), 1)


def _events(frame, cls, doas):
    doas = np.asarray(doas, dtype=np.float64).reshape(len(doas), -1)
    return np.concatenate((np.full((len(doas), 1), float(frame)), np.full((len(doas), 1), float(cls)), doas), 1)


def cell_deg(seed, g, q, jitter=8.0, az_off=22.0, el_off=8.0):
    """(references (g, 2), predictions (q, 2)) in degrees: max(g, q) of the BASE directions in a seeded order, jittered;
    each prediction a reference moved by 3 .. az_off degrees of azimuth and up to el_off of elevation, the predictions in
    the reverse order of their references."""
    n = max(g, q)
    order = np.argsort(uniform(seed, (8,)), kind="stable")[:n]
    ref = BASE[order] + (2.0 * uniform(seed + 1, (n, 2)) - 1.0) * jitter
    u = uniform(seed + 2, (n, 3))
    move = np.stack((np.where(u[:, 2] < 0.5, -1.0, 1.0) * (3.0 + (az_off - 3.0) * u[:, 0]), (2.0 * u[:, 1] - 1.0) * el_off), 1)
    pred = (ref + move)[::-1]
    return ref[:g], pred[:q]


def _recording(cells, coords):
    """cells: [(frame, class, ref_deg, pred_deg)] -> (pred rows, true rows), frames ascending, of the asked width."""
    conv = (lambda d: d) if coords == 2 else to_xyz
    cells = sorted(cells, key=lambda c: c[0])
    P = [_events(f, c, conv(p)) for f, c, r, p in cells if len(p)]
    T = [_events(f, c, conv(r)) for f, c, r, p in cells if len(r)]
    return (np.concatenate(P) if P else empty(coords)), (np.concatenate(T) if T else empty(coords))


def _case(name, kind, coords, max_tracks, pred, true, n_frames, fpb=10, nb_classes=14):
    return dict(name=name, kind=kind, coords=coords, max_tracks=max_tracks, pred=pred, true=true, n_frames=n_frames, fpb=fpb,
                nb_classes=nb_classes, doa_threshold=20.0, spatial_threshold=2.0)


def _general_cells(seed, n_frames):
    """Cells of at most 3 x 3 over 14 classes: about a third of the (frame, class) positions, sides of 0 .. 3 events."""
    cells = []
    u = uniform(seed, (n_frames, 14, 3))
    for f in range(n_frames):
        for c in range(14):
            if u[f, c, 0] > 0.35:
                continue
            g, q = int(u[f, c, 1] * 4), int(u[f, c, 2] * 4)
            if g + q:
                cells.append((f, c) + cell_deg(seed + 1000 + 97 * f + 7 * c, g, q))
    return cells


def _track_cells():
    """20 frames x 4 classes: every (g, q) of TRACK_COUNTS squared once, then cells with one side only."""
    shapes = [(g, q) for g in TRACK_COUNTS for q in TRACK_COUNTS] + [(1, 0), (0, 2), (4, 0), (0, 5), (8, 0), (0, 8), (2, 0)]
    cells = []
    for k, (g, q) in enumerate(shapes):
        f, c = (k * 7) % 20, (k // 3) % 4               # a seeded-looking but fixed spread over frames and classes
        while any(cell[0] == f and cell[1] == c for cell in cells):
            f = (f + 1) % 20
        cells.append((f, c) + cell_deg(3000 + 31 * k, g, q))
    return cells


def _degenerate_cells():
    d = lambda *rows: np.asarray(rows, dtype=np.float64).reshape(-1, 2)      # noqa: E731
    return [
        (0, 0, d([179.0, 10.0]), d([-179.0, 10.0])),              # the +-180 wrap: 2 degrees of azimuth apart
        (1, 1, d([30.0, 90.0]), d([-100.0, 90.0])),               # both at the north pole: identical
        (2, 2, d([30.0, -90.0]), d([45.0, 90.0])),                # pole to pole: antipodal
        (3, 3, d([45.0, 20.0]), d([45.0, 20.0])),                 # identical
        (4, 4, d([10.0, 20.0]), d([-170.0, -20.0])),              # antipodal
        (5, 5, d([180.0, 0.0]), d([-180.0, 0.0])),                # the same point, a whole turn apart
        (6, 6, d([179.5, -5.0], [0.0, 90.0]), d([0.0, 90.0], [-179.5, -5.0])),       # wrap and pole in one 2 x 2 cell
        (7, 7, d([-60.0, 0.0], [120.0, 0.0]), d([120.0, 0.0])),   # 2 x 1: identical beats antipodal
        (9, 0, d([0.0, -90.0]), d([77.0, -90.0])),                # both at the south pole
    ]


def _tie_cells(coords):
    """4- and 6-event cells with duplicated rows.  A duplicated reference is always matched by a duplicated prediction, so
    that every cheapest pairing gives every track the same distance."""
    cells = []
    for k, (n, dup_ref, dup_pred) in enumerate(((4, [(1, 2)], [(1, 2)]), (6, [(0, 1)], [(0, 1), (3, 4)]), (4, [], [(0, 3)]),
                                                (6, [(2, 5)], [(2, 5)]))):
        ref, pred = cell_deg(5000 + 17 * k, n, n)
        pred = pred[::-1].copy()                        # prediction i belongs to reference i again
        for a, b in dup_ref:
            ref[b] = ref[a]
        for a, b in dup_pred:
            pred[b] = pred[a]
        cells.append((2 * k + 1, k % 3, ref, pred[::-1].copy()))
    return cells


def build_cases():
    cases = []
    recs = [_recording(_general_cells(100 + 50 * r, 30), 2) for r in range(2)]
    cases.append(_case("sph_general", "general", 2, 3, [r[0] for r in recs], [r[1] for r in recs], 30))
    P, T = _recording(_degenerate_cells(), 2)
    cases.append(_case("sph_degenerate", "degenerate", 2, 3, [P], [T], 10))
    P, T = _recording(_track_cells(), 3)
    cases.append(_case("cart_tracks", "general", 3, 8, [P], [T], 20, nb_classes=4))
    dense = [(f, c) + cell_deg(7000 + 53 * f + 11 * c, 8, 8) for f in range(10) for c in range(14)]
    P, T = _recording(dense, 3)
    cases.append(_case("cart_dense", "general", 3, 8, [P], [T], 10))
    P, T = _recording(_track_cells(), 2)
    cases.append(_case("sph_tracks", "general", 2, 8, [P], [T], 20, nb_classes=4))
    P, T = _recording(_tie_cells(2), 2)
    cases.append(_case("ties", "ties", 2, 8, [P], [T], 10))
    P, T = _recording(_tie_cells(3), 3)
    cases.append(_case("ties_cart", "ties", 3, 8, [P], [T], 10))
    return cases


EVENT_METRIC_EX_CASES = build_cases()
EX_CASE_IDS = [c["name"] for c in EVENT_METRIC_EX_CASES]


def assign_problems(spherical):
    """One association problem for every (g, q) in 0 .. 8: (gt (81, 8, C), pred (81, 8, C), gt_counts, pred_counts), C = 3
    Cartesian or 2 spherical in RADIANS, padded with zeros."""
    C = 2 if spherical else 3
    gt, pred = np.zeros((81, 8, C)), np.zeros((81, 8, C))
    gn, qn = np.zeros(81, dtype=np.int32), np.zeros(81, dtype=np.int32)
    for b in range(81):
        g, q = b // 9, b % 9
        ref, pr = cell_deg(9000 + 29 * b + (500 if spherical else 0), g, q)
        if spherical:
            ref, pr = ref * np.pi / 180., pr * np.pi / 180.
        else:
            ref, pr = to_xyz(ref), to_xyz(pr)
        gt[b, :g], pred[b, :q], gn[b], qn[b] = ref, pr, g, q
    return gt, pred, gn, qn


def frame_dict(rec):
    """frame -> [[class, *doa, event] ...] with Python ints and floats, event = the position among the frame's events of
    the class: what segment_labels takes, for rows of either width."""
    d = {}
    for row in rec.tolist():
        lst = d.setdefault(int(row[0]), [])
        lst.append([int(row[1])] + row[2:] + [sum(1 for e in lst if e[0] == int(row[1]))])
    return d
