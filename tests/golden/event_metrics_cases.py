"""Case table of the event-list scoring (metrics.py task 2 and Dcase21_metrics.py of the reference), shared by the fixture
generator (make_golden_event_metrics.py, runs against the reference) and the tests.  Pure data + seeded inputs: the draws
are decode_cases.uniform, a counter hash in integer arithmetic.

A case is a dict: name, n_frames, fpb (frames per block), nb_classes, spatial_threshold, doa_threshold, and `pred` / `true`,
one (E, 5) float64 array [frame, class, x, y, z] per recording ((0, 5) for none).  `lsd` False: the case holds a frame
outside range(n_frames), which location_sensitive_detection answers with KeyError, so only the DCASE part is recorded."""
import numpy as np

from tests.golden.decode_cases import uniform

E0 = np.zeros((0, 5), dtype=np.float64)


def rows(*r):
    return np.asarray(r, dtype=np.float64).reshape(-1, 5)


def _xyz(seed, n, scale=2.0):
    return (2.0 * uniform(seed, (n, 3)) - 1.0) * scale


def _near(xyz, seed, spread):
    """Positions `spread` (metres per axis, at most) away from xyz."""
    return xyz + (2.0 * uniform(seed, xyz.shape) - 1.0) * spread


def _events(frames, classes, xyz):
    return np.concatenate((np.asarray(frames, dtype=np.float64)[:, None], np.asarray(classes, dtype=np.float64)[:, None],
                           np.asarray(xyz, dtype=np.float64)), 1)


def decoded(seed, recordings, frames, density, classes=14, overlaps=3, max_loc=2.0):
    """What gen_submission_list_task2 returns first for seeded dense float32 (sed, doa): a list of (E, 5) float64 arrays
    (the generator checks them against the reference's function)."""
    n = classes * overlaps
    out, dense = [], []
    for r in range(recordings):
        u = uniform(seed + 7 * r, (frames, n))
        sed = np.where(u < density, 0.75, 0.25 * u).astype(np.float32)
        doa = (2.0 * uniform(seed + 7 * r + 3, (frames, 3 * n)) - 1.0).astype(np.float32)
        f, j = np.nonzero(np.round(sed) != 0)
        loc = (doa * np.float32(max_loc)).reshape(frames, n, 3)[f, j].astype(np.float64)
        out.append(_events(f, j // overlaps, loc) if f.size else E0)
        dense.append((sed, doa))
    return out, dense


def shuffle_frames(rec, seed):
    """The rows of a recording with its frames in another order; rows of one frame stay together and in order."""
    if rec.shape[0] == 0:
        return rec
    frames = np.unique(rec[:, 0])
    order = frames[np.argsort(uniform(seed, (frames.size,)), kind="stable")]
    return np.concatenate([rec[rec[:, 0] == f] for f in order])


def _case(name, pred, true, n_frames, fpb=10, nb_classes=14, spatial_threshold=2.0, doa_threshold=20.0, lsd=True):
    return dict(name=name, pred=pred, true=true, n_frames=n_frames, fpb=fpb, nb_classes=nb_classes,
                spatial_threshold=spatial_threshold, doa_threshold=doa_threshold, lsd=lsd)


def _overlap_block(seed, frames, shapes, n_frames, cls_of=lambda k: k % 14, spread=0.25):
    """Per frame `f` of `frames` and per (class index k, (g, q)) of `shapes[f]`: g references and q predictions of class
    cls_of(k), the predictions near the references (or anywhere when there are more of them)."""
    P, T = [], []
    for fi, f in enumerate(frames):
        for k, (g, q) in enumerate(shapes[fi % len(shapes)]):
            s = seed + 101 * fi + 13 * k
            ref = _xyz(s, max(g, q))
            T.append(_events([f] * g, [cls_of(k)] * g, ref[:g]))
            P.append(_events([f] * q, [cls_of(k)] * q, _near(ref, s + 1, spread)[::-1][:q]))
    return np.concatenate(P) if P else E0, np.concatenate(T) if T else E0


def build_cases():
    cases = []
    # (a) n_frames = 12, one recording: both sides empty, predictions only, references only
    some = _events([0, 3, 3, 11], [1, 2, 2, 13], _xyz(1, 4))
    cases += [_case("a_empty", [E0], [E0], 12), _case("a_pred_only", [some], [E0], 12), _case("a_true_only", [E0], [some], 12)]
    # (b) one frame: only predictions, then only references (FP / FN doubled)
    one = _events([0, 0, 0], [4, 4, 9], _xyz(2, 3))
    cases += [_case("b_pred_frame", [one], [E0], 1), _case("b_true_frame", [E0], [one], 1)]
    # (c) two references of one class near one prediction: p - matched = -1
    ref = _xyz(3, 1)
    cases.append(_case("c_negative_fp", [_events([5], [6], ref)],
                       [_events([5, 5], [6, 6], np.concatenate((_near(ref, 4, 0.1), _near(ref, 5, 0.1))))], 12))
    # (d) a frame longer than a wave.  d_70_both: 70 events in frame 1 over the 14 classes, 3 predictions and 2 references of
    # each; d_70_each: 70 rows in each list, 3 per class in 14 scored classes and 2 per class in 14 classes above nb_classes
    P, T = _overlap_block(6, [1], [[(2, 3)] * 14], 2)
    cases.append(_case("d_70_both", [P], [T], 2))
    P, T = _overlap_block(7, [1], [[(3, 3)] * 14 + [(2, 2)] * 14], 2, cls_of=lambda k: k)
    cases.append(_case("d_70_each", [P], [T], 2))
    # (e) three recordings, the middle one empty on both sides
    P0, T0 = _overlap_block(8, [0, 4, 9, 10, 19], [[(1, 1), (2, 1)], [(1, 2)]], 20)
    P2, T2 = _overlap_block(9, [2, 3, 15], [[(1, 1)], [(2, 2), (1, 0), (0, 1)]], 20)
    cases.append(_case("e_middle_empty", [P0, E0, P2], [T0, E0, T2], 20))
    # (f) events on both sides of every 64-frame boundary
    for n in (65, 129):
        fr = [f for f in (0, 62, 63, 64, 65, 126, 127, 128) if f < n]
        P, T = _overlap_block(10 + n, fr, [[(1, 1), (1, 2)], [(2, 1)], [(1, 1), (0, 1), (1, 0)]], n)
        cases.append(_case(f"f_frames_{n}", [P], [T], n))
    # (g) n_frames = 25, 10 frames a block: frame 27 lies in the last block (DCASE counts it), beyond range(25) (KeyError)
    P, T = _overlap_block(20, [3, 24, 27], [[(1, 1), (2, 1)], [(1, 1)], [(1, 2), (1, 1)]], 25)
    cases.append(_case("g_frame_27", [P], [T], 25, lsd=False))
    cases.append(_case("g_without_27", [P[P[:, 0] != 27]], [T[T[:, 0] != 27]], 25))
    # (h) association shapes 1x3, 3x1, 2x3, 3x3 ... over the frames of one block; tracks appear and vanish
    shapes = [[(1, 3), (3, 1), (2, 3), (3, 3)], [(3, 3), (1, 1), (3, 2), (0, 2)], [(2, 2), (0, 0), (1, 3), (3, 3)],
              [(0, 1), (2, 1), (3, 3), (1, 0)]]
    P, T = _overlap_block(30, [10, 11, 13, 14, 17, 19, 20, 22], shapes, 30, spread=0.6)
    cases.append(_case("h_overlaps", [P], [T], 30))
    # (i) classes 14 and 20 beside scored ones: ignored by the block metrics, counted by the detection
    P, T = _overlap_block(40, [1, 2, 7], [[(1, 1), (1, 1), (2, 1), (1, 2)]], 10, cls_of=lambda k: (3, 14, 20, 13)[k])
    cases.append(_case("i_high_classes", [P], [T], 10))
    # (j) a zero coordinate vector: 90 degrees from anything
    cases.append(_case("j_zero_vector", [rows([2, 5, 0, 0, 0], [3, 5, 1.0, 0.5, -0.2], [4, 1, 0, 0, 0])],
                       [rows([2, 5, 0.3, -1.2, 0.4], [3, 5, 0, 0, 0], [4, 1, 0, 0, 0])], 10))
    # (k) 20 recordings x 100 frames of gen_submission_list_task2 rows, 5 % and 30 % of the slots active; (l) the same
    # lists with the frames of every recording shuffled
    for tag, density, seed in (("05", 0.05, 50), ("30", 0.30, 60)):
        P, _ = decoded(seed, 20, 100, density)
        T, _ = decoded(seed + 1000, 20, 100, density)
        cases.append(_case("k_decoded_" + tag, P, T, 100))
        cases.append(_case("l_shuffled_" + tag, [shuffle_frames(r, seed + i) for i, r in enumerate(P)],
                           [shuffle_frames(r, seed + 500 + i) for i, r in enumerate(T)], 100))
    # (m) a block with more rows than the kernel stages in LDS (256 a side): 14 classes x 3 x 10 frames
    P, T = _overlap_block(70, list(range(10)), [[(3, 3)] * 14], 10, spread=0.5)
    cases.append(_case("m_420_rows_a_block", [P], [T], 10))
    return cases


EVENT_METRIC_CASES = build_cases()
CASE_IDS = [c["name"] for c in EVENT_METRIC_CASES]
SEGMENT_CASES = ("g_frame_27", "h_overlaps", "k_decoded_05")     # segment_labels structures recorded for these


def frame_dict(rec):
    """The per-frame dictionary gen_submission_list_task2 returns second, rebuilt from rows: frame -> [[class, x, y, z,
    event] ...] with Python ints and floats, event = the position among the frame's events of the class."""
    d = {}
    for f, c, x, y, z in rec.tolist():
        lst = d.setdefault(int(f), [])
        lst.append([int(c), x, y, z, sum(1 for e in lst if e[0] == int(c))])
    return d


def host_function_inputs():
    """Seeded arguments for the host functions: (Cartesian pairs (N, 6), spherical (N, 4) in radians, error lists)."""
    cart = np.concatenate((_xyz(80, 16), _xyz(81, 16)), 1)
    cart[3, :3] = 0.0
    cart[5, 3:] = cart[5, :3]
    sph = (uniform(82, (16, 4)) - 0.5) * np.array([2 * np.pi, np.pi, 2 * np.pi, np.pi])
    errs = uniform(83, (8, 4)) * np.array([1.0, 1.0, 180.0, 1.0])
    return cart, sph, errs
