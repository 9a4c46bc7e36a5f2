"""hip_ops.window_batch / hip_ops.ensemble_combine (csrc/ensemble.hip) and train.predict_recordings /
evaluate_recordings against the numpy statement of include/seld_hip.h in tests/ensemble_ref.py.

window_batch moves data, flips signs and adds one fp32 constant: every comparison is torch.equal, against the reference
AND against the composition it replaces (hip_ops.segment, then hip_ops.gather_rows_aug with a one-row table at
p_swap = 1): the existing kernels define the bytes.

ensemble_combine sums in fp32: |out - ref| <= (2N + 4) * 2^-24 * max|v| with N the members covering the frame (N
products, two N-term sums, one division) against the float64 reference.  Largest error / bound per case, MI355X:

    (R, S, K, T_out, hop_out, frames, classes, O)    uniform   triangular
    planted (1, 1, 1, 8, 8, 8, 14, 3)                0.000     0.183
    planted (2, 4, 16, 8, 4, 19, 14, 3)              0.076     0.097
    planted (2, 3, 8, 8, 8, 24, 14, 2)               0.096     0.130
    planted (1, 5, 16, 8, 3, 20, 1, 3)               0.063     0.063
    planted (1, 2, 4, 8, 4, 12, 14, 1)               0.114     0.137
    planted (1, 18, 16, 64, 32, 600, 14, 3)          0.083     0.083
    random  (2, 4, 16, 8, 4, 19, 14, 3)                        0.048    (no cell left out)
    random  (1, 18, 16, 64, 32, 600, 14, 3)                    0.073    (17 of 8400 cells left out)
    predict_recordings, tiny_DQ, K = 8, S = 4                  0.112    (no cell left out)
"""
import functools
import os
import pickle
import types

import numpy as np
import pytest
import torch

from tests import ensemble_ref as E
from tests.golden.cases import MODEL_CASES, metric_inputs
from tests.helpers import build_model, pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -7.5
GUARD = 8


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- window_batch -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _recordings(shape):
    rng = np.random.default_rng(sum(shape))
    x = rng.uniform(-3.0, 3.0, shape).astype(np.float32)
    x[:, :, 0, ::5] = 0.0                                   # flip 2 at its tie
    return x, _dev(x)


def _composition(xd, T, hop, S, table, first, count):
    """Members [first, first + count) by the existing kernels: segment the recordings, then one forced transform each."""
    H = pkg().hip_ops
    R, C, F, _ = xd.shape
    seg = H.segment(xd, T, hop, segments=S)                                 # (S, R, C, F, T)
    rows = seg.permute(1, 0, 2, 3, 4).contiguous().view(R * S, C, F, T)
    K = 1 if table is None else len(table)
    out = torch.empty((count, C, F, T), device=DEV)
    epoch = torch.zeros(1, device=DEV, dtype=torch.int32)
    for b in range(count):
        m = first + b
        aug = H.Augment(device=DEV) if table is None else H.Augment(table=table[m % K:m % K + 1], p_swap=1.0, device=DEV)
        H.gather_rows_aug(rows, None, torch.tensor([m // K], device=DEV), out[b:b + 1], None, epoch=epoch, seed=1, augment=aug)
    return out


def _window_case(shape, T, hop, table, first, count, B, offset=0):
    """One call into a sentinel-filled buffer (its data pointer `offset` floats past a 16-byte boundary) with guard words
    behind it, against the reference and the composition; returns the device rows."""
    H = pkg().hip_ops
    x, xd = _recordings(shape)
    R, C, F, L = shape
    S = H.window_count(L, T, hop)
    row = C * F * T
    flat = torch.full((offset + B * row + GUARD,), SENTINEL, device=DEV)
    out = flat[offset:offset + B * row].view(B, C, F, T)
    assert out.data_ptr() % 16 == (4 * offset) % 16
    got = H.window_batch(xd, out, seg_len=T, hop=hop, segments=S, table=table, first=first, count=count)
    assert got is out
    n = min(B, R * S * (1 if table is None else len(table)) - first) if count is None else count
    want = E.window_batch(x, np.full((B, C, F, T), SENTINEL, np.float32), seg_len=T, hop=hop, segments=S, table=table,
                          first=first, count=count)
    assert torch.equal(out.cpu(), torch.from_numpy(want)), (shape, first, count)
    assert (out[n:] == SENTINEL).all() and (flat[:offset] == SENTINEL).all() and (flat[offset + B * row:] == SENTINEL).all()
    assert torch.equal(out[:n], _composition(xd, T, hop, S, table, first, n)), (shape, first, count)
    return out


RAGGED, ALIGNED = (2, 8, 5, 37), (2, 8, 4, 64)


@pytest.mark.parametrize("shape, offset", [(RAGGED, 0), (ALIGNED, 0), (ALIGNED, 1)], ids=["ragged", "float4", "float4_offset"])
def test_window_batch_equals_the_reference_and_the_composition(shape, offset):
    """(R, C, F, L) = (2, 8, 5, 37) with T 16, hop 8: the scalar path and the tail padding; (2, 8, 4, 64): the float4
    path; the same into a buffer one float past a 16-byte boundary: the scalar path.  The 16-row phase preset (C = 8,
    flip 2), `first` no multiple of K, count < B with sentinel rows and guard words, the last members, no table."""
    H = pkg().hip_ops
    table = H.foa_transforms(mics=1, phase=True)
    assert table.shape == (16, 22) and (table[:, 8:16] == 2).any()
    S = H.window_count(shape[3], 16, 8)
    M = shape[0] * S * 16
    assert S == (4 if shape is RAGGED else 7)
    for first, count, B in ((0, 12, 12), (21, 9, 12), (M - 16, 12, 12), (M - 5, None, 12), (S * 16 - 3, 6, 6)):
        out = _window_case(shape, 16, 8, table, first, count, B, offset)
        if shape is RAGGED and first == M - 16:
            # the last window holds 13 frames and 3 of padding; under x -> -x, y -> -y (row 3) the padded phase is PI_F
            last = out[3]
            assert table[3, 8:16].tolist() == [0, 0, 0, 0, 0, 2, 0, 2]
            assert (last[5, :, 13:] == float(np.float32(np.pi))).all() and (last[4, :, 13:] == 0).all()
    for first, count, B in ((0, None, 5), (3, 4, 6), (shape[0] * S - 2, 2, 3)):
        _window_case(shape, 16, 8, None, first, count, B, offset)


def test_window_batch_refuses_what_it_cannot_do():
    H, L = pkg().hip_ops, pkg()._lib
    _, xd = _recordings(ALIGNED)
    out = torch.full((4, 8, 4, 16), SENTINEL, device=DEV)
    table = H.foa_transforms(mics=1, phase=True)
    for kw in (dict(first=-1), dict(first=7 * 2 * 16 - 3, count=4), dict(count=5), dict(count=0), dict(hop=0),
               dict(table=H.foa_transforms())):
        with pytest.raises(L.SeldHipError):
            H.window_batch(xd, out, **dict(dict(seg_len=16, hop=8, segments=7, table=table), **kw))
    with pytest.raises(L.SeldHipError):
        H.window_batch(xd, out[:, :, :, :8], seg_len=8, hop=8, segments=8)                 # not contiguous
    with pytest.raises(L.SeldHipError):
        H.window_batch(xd, out, seg_len=32, hop=8, segments=7)                             # another window length
    assert (out == SENTINEL).all()


# ---- ensemble_combine -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table(K):
    return E.table_for(K, pkg().hip_ops.foa_transforms)


@functools.lru_cache(maxsize=None)
def _planted(shape):
    return E.planted(shape, _table(shape[2]))


def _combine(shape, sed, doa, kind, align=True, perm=True):
    R, S, K, T_out, hop_out, frames, classes, O = shape
    return pkg().hip_ops.ensemble_combine(sed, doa, recordings=R, segments=S, hop_out=hop_out, frames=frames, classes=classes,
                                          overlaps=O, table=_table(K), window=kind, align=align, return_perm=perm)


def _reference(shape, sed, doa, kind, align=True):
    R, S, K, T_out, hop_out, frames, classes, O = shape
    return E.combine(sed, doa, recordings=R, segments=S, hop_out=hop_out, frames=frames, classes=classes, overlaps=O,
                     win=E.window_weights(kind, T_out), table=_table(K), align=align)


def _ratio(got_sed, got_doa, ref, peak, keep=None):
    """Largest |out - ref| / bound over the cells `keep` (R, frames, classes) bool."""
    R, frames, n = ref["sed"].shape
    bound = E.bound(ref["members"], peak)
    classes = ref["ambiguous"].shape[2]
    worst = 0.0
    for got, want in ((got_sed, ref["sed"]), (got_doa, ref["doa"])):
        err = np.abs(got.double().cpu().numpy() - want) / bound
        err = err.reshape(R, frames, classes, -1).max(-1)
        worst = max(worst, float(err[keep].max() if keep is not None else err.max()))
    return worst


@pytest.mark.parametrize("shape", E.PLANTED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_combine_recovers_the_planted_field(shape):
    """Members = a field + noise <= 0.01, slots shuffled per (member, frame, class), transformed by their row
    (tests/ensemble_ref.planted; no cell is ambiguous, none is left out).  perm equals the reference's everywhere and is
    -1 past `frames`; at least half of the cells with a choice hold a member that needed another pairing than the
    identity; the outputs are within the bound of the reference and within 0.011 + the bound of the field in the
    anchor's slot order; without the alignment at least half of those cells are off the field by more than 0.1; two
    runs give the same bytes; under both windows."""
    R, S, K, T_out, hop_out, frames, classes, O = shape
    case = _planted(shape)
    sed, doa = _dev(case["sed"]), _dev(case["doa"])
    peak = max(np.abs(case["sed"]).max(), np.abs(case["doa"]).max())
    for kind in ("uniform", "triangular"):
        ref = _reference(shape, case["sed"], case["doa"], kind)
        assert not ref["ambiguous"].any()
        got_sed, got_doa, perm = _combine(shape, sed, doa, kind)
        assert got_sed.shape == (R, frames, classes * O) and got_doa.shape == (R, frames, 3 * classes * O)
        assert perm.dtype == torch.int32 and torch.equal(perm.cpu(), torch.from_numpy(ref["perm"]))
        past = (np.arange(S)[:, None] * hop_out + np.arange(T_out)[None, :]) >= frames              # (S, T_out)
        p5 = perm.cpu().numpy().reshape(R, S, K, T_out, classes)
        assert (p5[:, past.nonzero()[0], :, past.nonzero()[1]] == -1).all() and (p5.transpose(0, 1, 3, 2, 4)[:, ~past] >= 0).all()
        ratio = _ratio(got_sed, got_doa, ref, peak)
        print(f"planted {shape} {kind}: max error / bound = {ratio:.3f}")
        assert ratio <= 1.0
        ts, td = E.truth_for(case, shape, E.window_weights(kind, T_out))
        bound = E.bound(ref["members"], peak)
        assert (np.abs(got_sed.double().cpu().numpy() - ts) <= 0.011 + bound).all()
        assert (np.abs(got_doa.double().cpu().numpy() - td) <= 0.011 + bound).all()
        again = _combine(shape, sed, doa, kind)
        assert all(torch.equal(a, b) for a, b in zip(again, (got_sed, got_doa, perm)))
        no_perm = _combine(shape, sed, doa, kind, perm=False)
        assert len(no_perm) == 2 and torch.equal(no_perm[0], got_sed) and torch.equal(no_perm[1], got_doa)
        plain_sed, plain_doa, plain_perm = _combine(shape, sed, doa, kind, align=False)
        live = torch.from_numpy(ref["perm"] >= 0)
        assert (plain_perm.cpu()[live] == 0).all() and (plain_perm.cpu()[~live] == -1).all()
        if O > 1 and S * K > 1:                             # cells with a choice
            moved = np.zeros((R, frames, classes), dtype=bool)
            for s in range(S):
                j = np.arange(T_out)[s * hop_out + np.arange(T_out) < frames]
                moved[:, s * hop_out + j] |= (p5[:, s][:, :, j] > 0).any(1)
            assert moved.mean() >= 0.5
            off = np.maximum(np.abs(plain_sed.double().cpu().numpy() - ts).reshape(R, frames, classes, -1).max(-1),
                             np.abs(plain_doa.double().cpu().numpy() - td).reshape(R, frames, classes, -1).max(-1))
            assert (off > 0.1).mean() >= 0.5
        else:                                               # one slot or one member: nothing to align
            assert torch.equal(plain_sed, got_sed) and torch.equal(plain_doa, got_doa)


@pytest.mark.parametrize("shape", E.RANDOM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_combine_on_random_members(shape):
    """sed uniform in (0, 1), doa in (-1, 1): the members of a cell have nothing in common and the permutations' costs
    are close.  Entries of perm the reference marks ambiguous (second-best within 1e-4) are left out of the perm check,
    their cells out of the value check (none at the small shape; tests/test_ensemble_host.py holds the counts)."""
    sed, doa = E.uniform_members(shape, E.RANDOM_SEEDS[shape])
    ref = _reference(shape, sed, doa, "triangular")
    got_sed, got_doa, perm = _combine(shape, _dev(sed), _dev(doa), "triangular")
    keep = ~ref["ambiguous_members"]
    assert np.array_equal(perm.cpu().numpy()[keep], ref["perm"][keep])
    ratio = _ratio(got_sed, got_doa, ref, 1.0, ~ref["ambiguous"])
    print(f"random {shape}: max error / bound = {ratio:.3f}, {int(ref['ambiguous'].sum())} of {ref['ambiguous'].size} cells left out")
    assert ratio <= 1.0
    again = _combine(shape, _dev(sed), _dev(doa), "triangular")
    assert all(torch.equal(a, b) for a, b in zip(again, (got_sed, got_doa, perm)))


def test_combine_uncovered_frames_custom_weights_and_refusals():
    H, L = pkg().hip_ops, pkg()._lib
    shape = (1, 2, 4, 8, 4, 12, 14, 1)
    sed, doa = E.uniform_members(shape, 3)
    sd, dd = _dev(sed), _dev(doa)
    table = _table(4)
    # frames beyond the last window: zeros; weights of the caller's
    win = np.array([0.5, 1, 2, 4, 4, 2, 1, 0.25], np.float32)
    got = H.ensemble_combine(sd, dd, recordings=1, segments=2, hop_out=4, frames=15, classes=14, overlaps=1, table=table,
                             window=torch.from_numpy(win), return_perm=True)
    ref = E.combine(sed, doa, recordings=1, segments=2, hop_out=4, frames=15, classes=14, overlaps=1, win=win, table=table)
    assert ref["members"].tolist() == [4] * 4 + [8] * 4 + [4] * 4 + [0] * 3
    assert not got[0][0, 12:].any() and not got[1][0, 12:].any() and _ratio(got[0], got[1], ref, 1.0) <= 1.0
    assert torch.equal(got[2].cpu(), torch.from_numpy(ref["perm"]))
    for kw in (dict(window=[1.0] * 7), dict(window=[1.0] * 7 + [0.0]), dict(window=[1.0] * 7 + [float("nan")]),
               dict(window="hann"), dict(segments=3), dict(frames=0), dict(hop_out=0), dict(classes=7),
               dict(table=E.hand_table(4)[:, :-1])):
        with pytest.raises(L.SeldHipError):
            H.ensemble_combine(sd, dd, **dict(dict(recordings=1, segments=2, hop_out=4, frames=12, classes=14, overlaps=1,
                                                   table=table), **kw))
    wide = torch.zeros((1, 8, 56), device=DEV), torch.zeros((1, 8, 168), device=DEV)
    with pytest.raises(L.SeldHipError):
        H.ensemble_combine(*wide, recordings=1, segments=1, hop_out=8, frames=8, classes=14, overlaps=4)
    out = H.ensemble_combine(*wide, recordings=1, segments=1, hop_out=8, frames=8, classes=14, overlaps=4, align=False)
    assert out[0].shape == (1, 8, 56) and not out[0].any()


# ---- the model level --------------------------------------------------------------------------------------------------
class _Spread:
    """tiny_DQ in eval mode with its activities spread over both sides of one half (a fixed gain per output)."""

    def __init__(self):
        case = next(c for c in MODEL_CASES if c["name"] == "tiny_DQ")
        self.inner = build_model(case).to(DEV).eval()
        self.gain = _dev(np.random.default_rng(2).uniform(0.2, 1.8, 42).astype(np.float32))

    def eval(self):
        self.inner.eval()
        return self

    def __call__(self, x):
        sed, doa = self.inner(x)
        return sed * self.gain, doa


@functools.lru_cache(maxsize=None)
def _model():
    return _Spread()


@functools.lru_cache(maxsize=None)
def _model_input(L):
    x = np.random.default_rng(L).uniform(0.05, 1.05, (2, 8, 128, L)).astype(np.float32)
    return x, _dev(x)


def test_predict_recordings_equals_the_reference_on_the_models_own_outputs():
    """tiny_DQ (64 frames -> 8), two recordings of 160 frames, hop 32 (S = 4), the 8 transforms with z fixed, batch 8: the
    numpy combine of what the model gives for the same window_batch batches, to the bound.  Cells the reference marks
    ambiguous are left out; most cells must remain."""
    T, H = pkg().train, pkg().hip_ops
    model = _model()
    _, xd = _model_input(160)
    table = H.foa_transforms(mics=2, elevation=False)
    assert H.window_count(160, 64, 32) == 4
    sed, doa = T.predict_recordings(model, xd, seg_len=64, hop=32, table=table, batch=8)
    assert sed.shape == (2, 20, 42) and doa.shape == (2, 20, 126)
    xb = torch.zeros((8, 8, 128, 64), device=DEV)
    outs = []
    with torch.no_grad():
        for first in range(0, 64, 8):
            H.window_batch(xd, xb, seg_len=64, hop=32, segments=4, table=table, first=first)
            outs.append(tuple(t.clone() for t in model(xb[:8])))
    sed_m = torch.cat([o[0] for o in outs]).cpu().numpy()
    doa_m = torch.cat([o[1] for o in outs]).cpu().numpy()
    assert sed_m.shape == (64, 8, 42)
    ref = E.combine(sed_m, doa_m, recordings=2, segments=4, hop_out=4, frames=20, classes=14, overlaps=3,
                    win=E.window_weights("triangular", 8), table=table)
    keep = ~ref["ambiguous"]
    ratio = _ratio(sed, doa, ref, max(np.abs(sed_m).max(), np.abs(doa_m).max()), keep)
    print(f"predict_recordings: max error / bound = {ratio:.3f}, {int((~keep).sum())} of {keep.size} cells left out")
    assert keep.mean() >= 0.5 and ratio <= 1.0


def test_predict_recordings_without_overlap_or_transforms_is_the_models_output():
    T, H = pkg().train, pkg().hip_ops
    model = _model()
    _, xd = _model_input(128)
    sed, doa = T.predict_recordings(model, xd, seg_len=64, hop=64, window="uniform", batch=8)
    xb = torch.zeros((8, 8, 128, 64), device=DEV)
    with torch.no_grad():
        H.window_batch(xd, xb, seg_len=64, hop=64, segments=2, count=4)
        want_sed, want_doa = model(xb[:4])
    assert torch.equal(sed, want_sed.reshape(2, 16, 42)) and torch.equal(doa, want_doa.reshape(2, 16, 126))
    # chunks of one recording and a partial last batch give the same bytes
    old, pkg().evaluate.MEMBER_BUFFER_BYTES = T.MEMBER_BUFFER_BYTES, 1
    try:
        again = T.predict_recordings(model, xd, seg_len=64, hop=64, window="uniform", batch=8)
    finally:
        pkg().evaluate.MEMBER_BUFFER_BYTES = old
    assert torch.allclose(again[0], sed, atol=1e-5) and torch.allclose(again[1], doa, atol=1e-5)
    with pytest.raises(pkg()._lib.SeldHipError, match="multiple"):
        T.predict_recordings(model, xd, seg_len=64, hop=20)


def test_evaluate_recordings_scores_the_stitched_outputs(capsys):
    T, H = pkg().train, pkg().hip_ops
    model = _model()
    _, xd = _model_input(160)
    table = H.foa_transforms(mics=2, elevation=False)
    target = _dev(metric_inputs(2, 20, 41, "crowded")[2])
    args = types.SimpleNamespace(time_dim=64, class_overlaps=3, output_classes=14, Dcase21_metrics_DOA_threshold=20)
    results = T.evaluate_recordings(model, torch.device(DEV), xd, target, args, hop=32, table=table, epoch=7, batch=8, num_frames=20)
    assert "F score: " in capsys.readouterr().out
    assert len(results) == 16 and results[0] == 7
    sed, doa = T.predict_recordings(model, xd, seg_len=64, hop=32, table=table, batch=8, frames=20)
    dense = H.metrics_new(DEV)
    H.metrics_accumulate(dense, sed, doa, target, 20, 14, 3, 2., 2., 20)
    counts = dict(zip(H.METRIC_COUNTERS, dense[0].cpu().tolist()))
    want = T.test_results_from_counters(counts, float(dense[1].item()), 7)
    assert results[5:8] == want[5:8] and results == pytest.approx(want, rel=1e-9, abs=1e-12)
    pr, _, po = H.decode_events(sed, doa)
    tr, _, to = H.decode_events(target[..., :42].contiguous(), target[..., 42:].contiguous())
    acc = H.score_events(H.event_metrics_new(DEV), pr, po, tr, to, 20)
    assert acc[0][:13].tolist() == dense[0].tolist() and pr.shape[0] > 0 and results[5] + results[6] > 0
    assert abs(float(acc[1]) - float(dense[1])) <= 1e-9 * max(1.0, abs(float(dense[1])))


def _write_pickles(directory):
    rng = np.random.default_rng(5)
    paths = {}
    for split, n in (("training", 2), ("validation", 2), ("test", 2)):
        x = (rng.random((n, 8, 128, 64)) + 0.05).astype(np.float32)
        act = (rng.random((n, 8, 42)) < 0.15).astype(np.float32)
        loc = rng.uniform(-1, 1, (n, 8, 126)).astype(np.float32) * np.repeat(act, 3, axis=2)
        for kind, arr in (("predictors", x), ("target", np.concatenate([act, loc], axis=2))):
            paths[f"{split}_{kind}_path"] = os.path.join(str(directory), f"{split}_{kind}.pkl")
            with open(paths[f"{split}_{kind}_path"], "wb") as f:
                pickle.dump(arr, f)
    return paths


@pytest.mark.parametrize("extra, leg", [(dict(test_hop=0, test_tta=0), "evaluate_test"), (dict(test_tta=8), "evaluate_recordings")])
def test_main_takes_the_old_test_leg_unless_a_flag_is_set(tmp_path, monkeypatch, extra, leg):
    """One epoch of train.main on the tiny model with a test set and --test_step 1: with both flags 0 the test leg is
    evaluate_test and evaluate_recordings is never entered; --test_tta 8 alone runs whole-sample test-time augmentation."""
    from tests.test_gpu_train_loader import MODEL_FLAGS
    T = pkg().train
    called = []
    for name in ("evaluate_test", "evaluate_recordings"):
        def spy(*a, _name=name, _fn=getattr(T, name), **k):
            called.append((_name, k))
            return _fn(*a, **k)
        monkeypatch.setattr(T, name, spy)
    flags = dict(MODEL_FLAGS, **_write_pickles(tmp_path), results_path=str(tmp_path / "res"), checkpoint_dir=str(tmp_path / "ck"),
                 batch_size=2, epochs=1, min_n_epochs=1, **extra)
    flags.update(test_step=1)
    args = T.parse_args([f"--{k}={v}" for k, v in flags.items()])
    assert T.ensemble_requested(args) == (leg == "evaluate_recordings")
    T.main(args)
    assert [name for name, _ in called] == [leg]
    if leg == "evaluate_recordings":
        kw = called[0][1]
        assert kw["hop"] == 64 and kw["table"].shape == (8, 22)


def test_test_time_flips_of_standardised_phase_are_refused():
    T = pkg().train
    args = T.parse_args(["--TextArgs=none", "--test_tta=16", "--phase=True", "--input_channels=8"])
    with pytest.raises(ValueError, match="raw phase"):
        T.main(args)
    args = T.parse_args(["--TextArgs=none", "--test_tta=16", "--phase=True", "--input_channels=8", "--dataset_normalization=False"])
    assert T.ensemble_from_args(args)["table"].shape == (16, 22)
