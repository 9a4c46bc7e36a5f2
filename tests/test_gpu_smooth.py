"""hip_ops.smooth_tracks / hip_ops.track_events (csrc/smooth.hip) and the post-processed test legs of train.py against the
numpy statement of include/seld_hip.h in tests/smooth_ref.py.

The filtered activity and the 0 / 1 output are compared with np.array_equal: a median is an element of its window and the
run rules are integer logic.  The DOAs of inactive frames, and of every frame in "frame" mode, are the input's bits.  A
run's DOA is held to smooth_ref.bound on EVERY frame of EVERY run:  2^-24 |ref| + 4 * run length * 2^-53 * peak  (two
double sums, each within run length * 2^-53 relatively on the kernel's side and on the reference's, one division, one
rounding to fp32).  The rounding to fp32 alone uses up to 2^-24 |ref|, so the ratio comes close to 1 by construction; what
the sums add is the rest.  Largest error / bound over the random cases per T, MI355X:

    T          1      2      5      63     64     65     255    257    600    769    1025   16384
    mean       0.000  0.999  0.993  0.983  0.955  0.994  0.996  0.980  0.960  0.993  0.990  -
    weighted   0.000  0.924  0.958  0.907  0.962  0.996  0.951  0.970  0.953  0.978  0.998  0.985
    (T = 1: no event in a "mean" or "weighted" case; T = 16384 is one "weighted" case)
"""
import types

import numpy as np
import pytest
import torch

from tests import smooth_ref as S
from tests.golden.cases import metric_inputs
from tests.helpers import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.5
GUARD = 16
PLANTED = S.planted_cases()
MODE_CODE = {"frame": 0, "mean": 1, "weighted": 2}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(shape):
    """(flat, view): a sentinel-filled buffer with GUARD words on either side of the view."""
    numel = int(np.prod(shape))
    flat = torch.full((numel + 2 * GUARD,), SENTINEL, device=DEV)
    return flat, flat[GUARD:GUARD + numel].view(shape)


def _guards_intact(flat):
    return bool((flat[:GUARD] == SENTINEL).all() and (flat[-GUARD:] == SENTINEL).all())


def _raw(sed_d, doa_d, params, mode, prob=True):
    """seld_smooth_tracks into guarded, sentinel-filled outputs: (rc, out_sed, out_doa, out_prob, the three flat buffers)."""
    L = pkg()._lib
    R, T, n = sed_d.shape
    bufs = [_guarded((R, T, n)), _guarded((R, T, 3 * n)), _guarded((R, T, n))]
    with torch.cuda.device(DEV):
        rc = L.lib().seld_smooth_tracks(L.ptr(sed_d), L.ptr(doa_d), R, T, n, params["median"], params["on"], params["off"],
                                        params["min_frames"], params["max_gap"], MODE_CODE[mode], L.ptr(bufs[0][1]),
                                        L.ptr(bufs[1][1]), L.ptr(bufs[2][1] if prob else None), L.current_stream())
    return rc, bufs[0][1], bufs[1][1], bufs[2][1], [b[0] for b in bufs]


def _check_doa(got, doa, ref):
    """Every element of out_doa: the input's bits on inactive frames; on every frame of every run constant and within the
    bound of the reference.  Returns the largest error / bound."""
    got64 = got.astype(np.float64)
    tol = np.zeros_like(got64)
    active = np.zeros(got.shape, dtype=bool)
    for r, j, s, e, peak in ref["runs"]:
        cols = slice(3 * j, 3 * j + 3)
        tol[r, s:e, cols] = S.bound(ref["doa"][r, s, cols], e - s, peak)[None, :]
        active[r, s:e, cols] = True
        assert (got[r, s:e, cols] == got[r, s, cols]).all(), ("a run's DOA is not constant", r, j, s, e)
    assert np.array_equal(got.view(np.int32)[~active], doa.view(np.int32)[~active])
    err = np.abs(got64 - ref["doa"])
    assert (err <= tol).all(), float((err - tol).max())
    return float((err[active] / tol[active]).max()) if active.any() else 0.0


def _check_case(sed, doa, params, mode, ref):
    """One case through the entry point (guarded buffers, with and without out_prob) and through the wrapper."""
    H = pkg().hip_ops
    sd, dd = _dev(sed), _dev(doa)
    rc, out_sed, out_doa, out_prob, flats = _raw(sd, dd, params, mode)
    assert rc == 0 and all(_guards_intact(f) for f in flats)
    assert np.array_equal(out_prob.cpu().numpy(), ref["prob"])
    assert np.array_equal(out_sed.cpu().numpy(), ref["sed"])
    ratio = 0.0
    if mode == "frame":
        assert torch.equal(out_doa.view(torch.int32), dd.view(torch.int32))
    else:
        ratio = _check_doa(out_doa.cpu().numpy(), doa, ref)
    # without out_prob: the same bytes, and the third buffer untouched
    rc, sed2, doa2, prob2, flats2 = _raw(sd, dd, params, mode, prob=False)
    assert rc == 0 and torch.equal(sed2, out_sed) and torch.equal(doa2.view(torch.int32), out_doa.view(torch.int32))
    assert bool((flats2[2] == SENTINEL).all())
    # the wrapper: the same bytes again (two runs give the same bytes)
    got = H.smooth_tracks(sd, dd, doa=mode, return_prob=True, **params)
    assert torch.equal(got[0], out_sed) and torch.equal(got[1].view(torch.int32), out_doa.view(torch.int32))
    assert torch.equal(got[2], out_prob)
    # "frame" mode keeps the activity and copies the DOAs
    if mode != "frame":
        plain = H.smooth_tracks(sd, dd, doa="frame", **params)
        assert len(plain) == 2 and torch.equal(plain[0], out_sed) and torch.equal(plain[1].view(torch.int32), dd.view(torch.int32))
    return ratio


@pytest.mark.parametrize("case", PLANTED, ids=[c["name"] for c in PLANTED])
def test_planted_cases_give_their_literal_outputs(case):
    H = pkg().hip_ops
    mode = case["want_doa"][0] if case["want_doa"] else "frame"
    ref = S.smooth(case["sed"], case["doa"], doa_mode=mode, **case["params"])
    for m in S.DOA_MODES:
        _check_case(case["sed"], case["doa"], case["params"], m, ref if m == mode else
                    S.smooth(case["sed"], case["doa"], doa_mode=m, **case["params"]))
    out = H.smooth_tracks(_dev(case["sed"][0]), _dev(case["doa"][0]), doa=mode, return_prob=True, **case["params"])   # (T, n)
    assert out[0].shape == case["sed"].shape[1:] and np.array_equal(out[0].cpu().numpy(), case["want_sed"][0])
    if case["want_prob"] is not None:
        assert np.array_equal(out[2].cpu().numpy(), case["want_prob"][0])
    if case["want_doa"] is not None:
        assert np.array_equal(out[1].double().cpu().numpy(), case["want_doa"][1][0])     # exact: the sums are
    else:
        assert np.array_equal(out[1].cpu().numpy(), case["doa"][0])


@pytest.mark.parametrize("T", S.RANDOM_T + (S.MAX_FRAMES,))
def test_random_cases_equal_the_reference(T):
    """Every (R, n) at T frames (tests/smooth_ref.random_specs; at SMOOTH_MAX_FRAMES the one shape (1, T, 3)): filtered
    activity and output activity exact, DOAs as the module docstring says, guard words intact, the same bytes from a
    second and a third run."""
    specs = S.random_specs(T) if T != S.MAX_FRAMES else [S.longest_spec()]
    worst = {"mean": 0.0, "weighted": 0.0}
    for spec in specs:
        case = S.random_case(spec)
        ratio = _check_case(case["sed"], case["doa"], case["params"], case["doa_mode"], case["ref"])
        worst[case["doa_mode"]] = max(worst[case["doa_mode"]], ratio)
    print(f"T = {T}: largest error / bound: mean {worst['mean']:.3f}, weighted {worst['weighted']:.3f}")
    assert max(worst.values()) <= 1.0


def test_refused_calls_raise_and_write_nothing():
    H, L = pkg().hip_ops, pkg()._lib
    sed, doa = S.random_track(2, 40, 3, 5)
    sd, dd = _dev(sed), _dev(doa)
    good = dict(median=3, on=0.75, off=0.25, min_frames=2, max_gap=1)
    nan, inf = float("nan"), float("inf")
    for bad in (dict(median=2), dict(median=0), dict(median=33), dict(on=nan), dict(off=nan), dict(on=inf), dict(off=-inf),
                dict(on=0.25, off=0.75), dict(on=1.25), dict(off=-0.25), dict(min_frames=0), dict(max_gap=-1)):
        params = dict(good, **bad)
        rc, out_sed, out_doa, out_prob, flats = _raw(sd, dd, params, "mean")
        assert rc == -1 and all(bool((f == SENTINEL).all()) for f in flats), bad
        with pytest.raises(L.SeldHipError):
            H.smooth_tracks(sd, dd, doa="mean", **params)
    with pytest.raises(L.SeldHipError):
        H.smooth_tracks(sd, dd, doa="median", **good)
    lib = L.lib()
    out = [_guarded((2, 40, 3)), _guarded((2, 40, 9))]

    def call(sed=sd, doa=dd, R=2, T=40, n=3, mode=1, out_sed=out[0][1], out_doa=out[1][1]):
        return lib.seld_smooth_tracks(L.ptr(sed), L.ptr(doa), R, T, n, 3, 0.75, 0.25, 2, 1, mode, L.ptr(out_sed), L.ptr(out_doa),
                                      None, L.current_stream())
    for kw, rc in ((dict(sed=None), -1), (dict(doa=None), -1), (dict(out_sed=None), -1), (dict(out_doa=None), -1),
                   (dict(R=0), -1), (dict(T=0), -1), (dict(n=0), -1), (dict(mode=3), -1), (dict(mode=-1), -1),
                   (dict(T=S.MAX_FRAMES + 1), -4), (dict(R=1 << 31, n=1), -4), (dict(R=1 << 29, n=4), -4)):
        assert call(**kw) == rc, kw
        with pytest.raises(L.SeldHipError):
            L.check(call(**kw), "seld_smooth_tracks")
    torch.cuda.synchronize()
    assert all(bool((flat == SENTINEL).all()) for flat, _ in out)
    with pytest.raises(L.SeldHipError):                         # the wrapper's own checks
        H.smooth_tracks(torch.zeros((1, S.MAX_FRAMES + 1, 1), device=DEV), torch.zeros((1, S.MAX_FRAMES + 1, 3), device=DEV))
    for a, b in ((sd, dd[:, :, :6]), (sd.double(), dd.double()), (sd[0], dd), (sd.cpu(), dd.cpu()), (sd[:, :0], dd[:, :0])):
        with pytest.raises(L.SeldHipError):
            H.smooth_tracks(a, b, median=3)
    assert call() == 0                                          # the same call, unspoilt, runs
    torch.cuda.synchronize()
    assert np.array_equal(out[0][1].cpu().numpy(), S.smooth(sed, doa, **good)["sed"]) and _guards_intact(out[0][0])


def test_a_recorded_call_replayed_on_new_input_equals_the_eager_call():
    H = pkg().hip_ops
    rules = dict(median=3, on=0.5625, off=0.4375, min_frames=6, max_gap=2)
    params = dict(rules, doa="weighted", return_prob=True)
    first, second = S.random_track(3, 600, 42, 21), S.random_track(3, 600, 42, 22)
    sd, dd = _dev(first[0]), _dev(first[1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        H.smooth_tracks(sd, dd, **params)                       # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        static = H.smooth_tracks(sd, dd, **params)
    sd.copy_(_dev(second[0]))
    dd.copy_(_dev(second[1]))
    graph.replay()
    torch.cuda.synchronize()
    eager = H.smooth_tracks(_dev(second[0]), _dev(second[1]), **params)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(static, eager))
    ref = S.smooth(*second, doa_mode="weighted", **rules)
    assert np.array_equal(static[0].cpu().numpy(), ref["sed"]) and ref["filled"] and ref["short"] and ref["dropped"]
    assert not np.array_equal(ref["sed"], S.smooth(*first, **rules)["sed"])


@pytest.mark.parametrize("variant", ["crowded", "half_silent"])
def test_identity_settings_decode_to_the_same_events(variant):
    H = pkg().hip_ops
    sed, doa, _ = metric_inputs(3, 100, 17, variant)
    assert sed.min() >= 0 and sed.max() <= 1 and (sed == 0.5).any()
    sd, dd = _dev(sed), _dev(doa)
    assert H.PostProcess().is_identity
    smooth = H.smooth_tracks(sd, dd, **H.PostProcess().kwargs())
    assert torch.equal(smooth[0], (sd > 0.5).float()) and torch.equal(smooth[1].view(torch.int32), dd.view(torch.int32))
    want, got = H.decode_events(sd, dd), H.decode_events(*smooth)
    assert want[0].shape[0] > 0 and all(torch.equal(a, b) for a, b in zip(want, got))


# ---- track_events -----------------------------------------------------------------------------------------------------
def _events_case(sed, doa, max_loc=2., classes=14, overlaps=3):
    H = pkg().hip_ops
    rows, offsets = H.track_events(_dev(sed), _dev(doa), max_loc, classes, overlaps)
    want, want_offsets, info = S.events(sed, doa, max_loc, overlaps)
    assert rows.dtype == torch.float64 and offsets.dtype == torch.int64 and rows.shape == want.shape
    got = rows.cpu().numpy()
    assert np.array_equal(got[:, :5], want[:, :5]) and np.array_equal(offsets.cpu().numpy(), want_offsets)
    if len(info):
        run_len, peak = np.array([i[0] for i in info], np.float64), np.array([i[1] for i in info])
        tol = S.event_bound(want[:, 5:], run_len[:, None], peak[:, None], max_loc)
        assert (np.abs(got[:, 5:] - want[:, 5:]) <= tol).all()
        key = got[:, 0] * 1e12 + (got[:, 1] * overlaps + got[:, 2]) * 1e6 + got[:, 3]       # recording, column, onset
        assert (np.diff(key) > 0).all()
    return got, offsets


def test_track_events_lists_every_run():
    """Raw probabilities (64-frame segments and runs across them at T = 600, 65 and 1025; one column; 64 columns), the
    0 / 1 output of smooth_tracks, and the (T, n) form."""
    H = pkg().hip_ops
    for shape, seed, classes, overlaps in (((3, 600, 42), 31, 14, 3), ((1, 65, 1), 32, 1, 1), ((2, 1025, 64), 33, 16, 4),
                                           ((3, 5, 3), 34, 1, 3), ((1, 1, 42), 35, 14, 3)):
        sed, doa = S.random_track(*shape, seed)
        got, _ = _events_case(sed, doa, 2., classes, overlaps)
        if shape[1] >= 600:
            assert ((got[:, 3] // 64) != ((got[:, 4] - 1) // 64)).any()         # a run that leaves its segment
    sed, doa = S.random_track(3, 600, 42, 31)
    out = H.smooth_tracks(_dev(sed), _dev(doa), median=7, on=0.75, off=0.25, min_frames=3, max_gap=2, doa="mean")
    got, _ = _events_case(out[0].cpu().numpy(), out[1].cpu().numpy(), 1.5)
    ref = S.smooth(sed, doa, median=7, on=0.75, off=0.25, min_frames=3, max_gap=2)
    assert [(int(r[0]), int(r[1]) * 3 + int(r[2]), int(r[3]), int(r[4])) for r in got] == [q[:4] for q in ref["runs"]]
    rows, offsets = H.track_events(_dev(sed[0]), _dev(doa[0]))
    want, want_offsets, _ = S.events(sed[:1], doa[:1])
    assert np.array_equal(rows.cpu().numpy()[:, :5], want[:, :5]) and offsets.tolist() == want_offsets.tolist()


def test_track_events_of_a_silent_track_and_a_short_capacity():
    H, L = pkg().hip_ops, pkg()._lib
    silent = torch.full((2, 70, 42), 0.5, device=DEV)           # 0.5 is off
    rows, offsets = H.track_events(silent, torch.zeros((2, 70, 126), device=DEV))
    assert rows.shape == (0, 8) and offsets.tolist() == [0, 0, 0]
    sed, doa = S.random_track(2, 130, 6, 41)
    want, want_offsets, _ = S.events(sed, doa, 2., 3)
    E = want.shape[0]
    assert E > 8
    sd, dd = _dev(sed), _dev(doa)
    lib = L.lib()
    nbytes = lib.seld_track_events_workspace(2, 130, 6)
    ws = torch.empty(nbytes // 8, device=DEV, dtype=torch.int64)
    L.check(lib.seld_track_events_count(L.ptr(sd), 2, 130, 6, L.ptr(ws), nbytes, L.current_stream()), "count")
    assert int(ws[0].item()) == E
    capacity = E - 5
    flat = torch.full((E * 8 + GUARD,), SENTINEL, device=DEV, dtype=torch.float64)
    offs = torch.empty(3, device=DEV, dtype=torch.int64)
    L.check(lib.seld_track_events_write(L.ptr(sd), L.ptr(dd), 2, 130, 2, 3, 2.0, L.ptr(ws), nbytes, L.ptr(flat), capacity,
                                        L.ptr(offs), L.current_stream()), "write")
    assert np.array_equal(flat[:capacity * 8].view(capacity, 8).cpu().numpy()[:, :5], want[:capacity, :5])
    assert bool((flat[capacity * 8:] == SENTINEL).all()) and offs.tolist() == want_offsets.tolist()
    L.check(lib.seld_track_events_write(L.ptr(sd), L.ptr(dd), 2, 130, 2, 3, 2.0, L.ptr(ws), nbytes, None, 0, L.ptr(offs),
                                        L.current_stream()), "write")
    assert offs.tolist() == want_offsets.tolist()
    for a, b, kw in ((sd, dd, dict(num_classes=4)), (sd.double(), dd.double(), {}), (sd, dd[:, :, :9], {})):
        with pytest.raises(L.SeldHipError):
            H.track_events(a, b, 2., **dict(dict(num_classes=2, max_overlaps=3), **kw))


# ---- the test legs ------------------------------------------------------------------------------------------------------
def _spy(monkeypatch):
    """Record what hip_ops.smooth_tracks is given and gives while train.py runs."""
    H = pkg().hip_ops
    calls = []

    def spy(sed, doa, /, **kw):
        out = real(sed, doa, **kw)
        calls.append((sed.clone(), doa.clone(), kw, out))
        return out
    real = H.smooth_tracks
    monkeypatch.setattr(H, "smooth_tracks", spy)
    return calls


def _against_reference(call, post):
    sed, doa, kw, out = call
    assert kw == post.kwargs()
    three = sed.dim() == 3
    s, d = sed.cpu().numpy(), doa.cpu().numpy()
    ref = S.smooth(s if three else s[None], d if three else d[None], doa_mode=post.doa,
                   **{k: v for k, v in post.kwargs().items() if k != "doa"})
    got_sed, got_doa = (out[0] if three else out[0][None]).cpu().numpy(), (out[1] if three else out[1][None]).cpu().numpy()
    assert np.array_equal(got_sed, ref["sed"])
    _check_doa(got_doa, d if three else d[None], ref)
    return ref


def test_predict_test_post_processes_before_it_decodes(monkeypatch):
    """train.predict_test_post: predict_test keeps its pinned signature and launches nothing new."""
    from tests.test_gpu_ensemble import _model, _model_input
    T, H = pkg().train, pkg().hip_ops
    model = _model()
    x, _ = _model_input(160)
    loader = [(torch.from_numpy(x[:, :, :, :64].copy()), None), (torch.from_numpy(x[:1, :, :, 64:128].copy()), None)]
    plain = T.predict_test(model, torch.device(DEV), loader)
    calls = _spy(monkeypatch)
    for post in (None, H.PostProcess(), dict(median=1)):        # None and the identity launch nothing
        again = T.predict_test_post(model, torch.device(DEV), loader, post=post)
        assert all(np.array_equal(a, b) for a, b in zip(again, plain)) and len(again) == len(plain) and not calls
    post = H.PostProcess(median=3, on=0.6, off=0.4, min_frames=2, max_gap=1, doa="mean")
    got = T.predict_test_post(model, torch.device(DEV), loader, post=post)
    assert len(calls) == 2 and len(got) == 3
    refs = [_against_reference(c, post) for c in calls]
    assert sum(len(r["runs"]) for r in refs) > 0
    rows = []
    for _, _, _, out in calls:                                  # the rows are the decoder's of the post-processed track
        r, _, offsets = H.decode_events(out[0], out[1], 2., 14, 3)
        rows.extend(r.cpu().numpy()[a:b] for a, b in zip(offsets.tolist()[:-1], offsets.tolist()[1:]))
    assert all(np.array_equal(a, b) for a, b in zip(got, rows))
    assert any(a.shape != b.shape or not np.array_equal(a, b) for a, b in zip(got, plain))


def test_evaluate_recordings_scores_the_post_processed_track(monkeypatch, capsys):
    from tests.test_gpu_ensemble import _model, _model_input
    T, H = pkg().train, pkg().hip_ops
    model = _model()
    _, xd = _model_input(160)
    target = _dev(metric_inputs(2, 20, 41, "crowded")[2])
    args = types.SimpleNamespace(time_dim=64, class_overlaps=3, output_classes=14, Dcase21_metrics_DOA_threshold=20)
    common = dict(hop=32, table=None, epoch=3, batch=8, num_frames=20)
    calls = _spy(monkeypatch)
    plain = T.evaluate_recordings(model, torch.device(DEV), xd, target, args, **common)
    same = T.evaluate_recordings(model, torch.device(DEV), xd, target, args, post=H.PostProcess(), **common)
    assert same[5:8] == plain[5:8] and same == pytest.approx(plain, rel=1e-9, abs=1e-12)     # the angle sum is atomic
    assert not calls
    post = H.PostProcess(median=3, on=0.6, off=0.4, min_frames=3, max_gap=1, doa="weighted")
    results = T.evaluate_recordings(model, torch.device(DEV), xd, target, args, post=post, **common)
    assert "F score: " in capsys.readouterr().out and len(calls) == 1 and calls[0][0].shape == (2, 20, 42)
    ref = _against_reference(calls[0], post)
    assert len(ref["runs"]) > 0
    raw_sed, raw_doa = T.predict_recordings(model, xd, seg_len=64, hop=32, batch=8, frames=20)
    assert torch.equal(raw_sed, calls[0][0]) and torch.equal(raw_doa, calls[0][1])          # the un-post-processed outputs
    dense = H.metrics_new(DEV)
    H.metrics_accumulate(dense, calls[0][3][0], calls[0][3][1], target, 20, 14, 3, 2., 2., 20)
    want = T.test_results_from_counters(dict(zip(H.METRIC_COUNTERS, dense[0].cpu().tolist())), float(dense[1].item()), 3)
    assert results[5:8] == want[5:8] and results == pytest.approx(want, rel=1e-9, abs=1e-12)
    assert results[5:8] != plain[5:8]


def test_evaluate_test_reads_the_settings_from_args(monkeypatch, capsys):
    from tests.test_gpu_ensemble import _model, _model_input
    T, H = pkg().train, pkg().hip_ops
    model = _model()
    x, _ = _model_input(160)
    target = torch.from_numpy(metric_inputs(2, 8, 43, "crowded")[2])
    loader = [(torch.from_numpy(x[:, :, :, :64].copy()), target)]
    calls = _spy(monkeypatch)
    flags = ["--TextArgs=none", "--class_overlaps=3", "--output_classes=14"]
    plain = T.evaluate_test(model, torch.device(DEV), loader, num_frames=8, args=T.parse_args(flags))
    assert not calls
    args = T.parse_args(flags + ["--post_median=3", "--post_on=0.6", "--post_off=0.4", "--post_min_frames=2", "--post_doa=mean"])
    results = T.evaluate_test(model, torch.device(DEV), loader, num_frames=8, args=args)
    capsys.readouterr()
    assert len(calls) == 1
    _against_reference(calls[0], T.postprocess_from_args(args))
    dense = H.metrics_new(DEV)
    H.metrics_accumulate(dense, calls[0][3][0], calls[0][3][1], target.to(DEV), 8, 14, 3, 2., 2., 20)
    want = T.test_results_from_counters(dict(zip(H.METRIC_COUNTERS, dense[0].cpu().tolist())), float(dense[1].item()), 0)
    assert results[5:8] == want[5:8] and results == pytest.approx(want, rel=1e-9, abs=1e-12) and len(plain) == 16


@pytest.mark.parametrize("extra", [dict(), dict(test_tta=8)], ids=["evaluate_test", "evaluate_recordings"])
def test_main_hands_the_flags_to_either_test_leg(tmp_path, monkeypatch, extra):
    """One epoch of train.main on the tiny model with a test set and --test_step 1: with --post_* set the test leg, with or
    without --test_tta, sends its track through smooth_tracks with the flags' settings; with the defaults it never does."""
    from tests.test_gpu_ensemble import _write_pickles
    from tests.test_gpu_train_loader import MODEL_FLAGS
    T, H = pkg().train, pkg().hip_ops
    calls = _spy(monkeypatch)
    base = dict(MODEL_FLAGS, **_write_pickles(tmp_path), results_path=str(tmp_path / "res"), checkpoint_dir=str(tmp_path / "ck"),
                batch_size=2, epochs=1, min_n_epochs=1, test_step=1, **extra)
    T.main(T.parse_args([f"--{k}={v}" for k, v in base.items()]))
    assert not calls
    flags = dict(base, post_median=3, post_on=0.6, post_off=0.4, post_min_frames=2, post_max_gap=1, post_doa="mean",
                 results_path=str(tmp_path / "res2"), checkpoint_dir=str(tmp_path / "ck2"))
    args = T.parse_args([f"--{k}={v}" for k, v in flags.items()])
    T.main(args)
    want = H.PostProcess(median=3, on=0.6, off=0.4, min_frames=2, max_gap=1, doa="mean")
    assert len(calls) >= 1 and all(kw == want.kwargs() for _, _, kw, _ in calls)
    assert sum(c[0].shape[0] for c in calls) == 2               # the two test recordings, each once
    _against_reference(calls[0], want)
